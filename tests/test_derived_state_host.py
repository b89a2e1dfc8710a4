"""Host-side checks of the data the package derives from weights and keeps between calls (relation_detr_amd/derived.py): every
cache is listed, every signalled change of every source reaches the derived data, what a recording ledger pinned outlives the
caches' eviction, and the decision a graph takes before a replay.  CPU tensors only; needs neither a GPU nor the built library.

The contract: C1 eager freshness after any change torch signals, C2 pinning, C3 replay decision, C4 the
two calls for writes torch does not signal."""
import ast
import gc
import os
import weakref

import pytest
import torch
from torch import nn

from relation_detr_amd import _lib, ops
from relation_detr_amd.backbones.resnet import FrozenBatchNorm2d
from relation_detr_amd.ms_deform_attn import MultiScaleDeformableAttention
from relation_detr_amd.transformer import RelationTransformer, build_relation_transformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------ inventory
# Every place of the package that keeps state between calls or reads a tensor's version: "module.name" -> what it is and what it is
# derived from.  `kind` of a DerivedCache row is the kind its pins carry in a ledger (tests/test_gpu_derived_state.py asserts that a
# forward's ledger names every kind that applies).  A new cache fails test_inventory_lists_every_cache until it is listed here.
INVENTORY = {
    # identity-keyed weight-derived caches (derived.DerivedCache instances)
    "ops._FFN_PACKED": dict(kind="ffn_packed", sources="(linear1.weight, linear2.weight) of a feed-forward block"),
    "ops._LINEAR_PACKED": dict(kind="linear_packed", sources="one weight: [256,256] block, K halves, in_proj, class weight, query proj"),
    "ops._REL_PROJ_F32": dict(kind="rel_proj_f32", sources="pos_proj weight | bias of the relation embedding, one entry each"),
    "ms_deform_attn._MERGED_QUERY": dict(kind="merged_query_projection", sources="sampling_offsets / attention_weights weight AND bias"),
    "transformer._VALUE_PROJ": dict(kind="value_projection_batched", sources="every decoder layer's cross_attn.value_proj weight AND bias"),
    "backbones.resnet._SCALE_SHIFT": dict(kind="frozen_bn_scale_shift", sources="weight, bias, running_mean, running_var buffers (+ eps)"),
    # tables without a weight source
    "transformer.RelationTransformer._geometry_cache": dict(kind="level_geometry", sources="level shapes + device; pinned, never refreshed"),
    "ops._shape_cache": dict(kind="host table", sources="spatial_shapes, level_start_index tensors: identity + version"),
    "ops._window_ok_cache": dict(kind="host table", sources="the host copy of the level table (values)"),
    "ops._host_array_cache": dict(kind="host table", sources="the host copy of the level table (values)"),
}
# functions that read `._version`
VERSION_READERS = {
    "derived.stamp": "the one definition of what a cache observes of a source",
    "derived.replay_decision": "compares a pin's stamps with its sources before a replay",
    "derived.Ledger._unchanged": "the same comparison, each distinct source once, for the replay where nothing changed",
    "ops.host_levels": "ops._shape_cache: version + address of the two level tensors, beside their identity",
    "optim.FusedAdamW._gather": "not a cache of weights: contiguous copies of gradients, valid for one step",
    "optim.FusedAdamW._prepared_still_holds": "not a cache of weights: the check of those copies",
}
CACHE_CLASSES = ("DerivedCache", "_PackedWeightCache")


def _package_files():
    package = os.path.join(ROOT, "relation_detr_amd")
    for folder, dirs, names in sorted(os.walk(package)):
        dirs[:] = sorted(d for d in dirs if d != "__pycache__")
        below = os.path.relpath(folder, package)
        parts = [] if below == "." else below.split(os.sep)
        for file in sorted(names):
            if file.endswith(".py"):
                yield ".".join(parts + [file[:-3]]), os.path.join(folder, file)


def _target_names(node):
    targets = node.targets if isinstance(node, ast.Assign) else [node.target]
    for t in targets:
        for sub in ([t] if not isinstance(t, (ast.Tuple, ast.List)) else t.elts):
            if isinstance(sub, ast.Name):
                yield sub.id
            elif isinstance(sub, ast.Attribute):
                yield sub.attr


def _scan():
    """(sites, readers): "module[.Class].name" of every assignment to a name or attribute ending in `_cache`, every by-name attribute
    store of such a name (setattr / object.__setattr__) and every variable bound to a new cache object; "module.function" of every
    function or method whose body reads `._version`."""
    sites, readers = set(), set()
    for module, path in _package_files():
        with open(path) as f:
            tree = ast.parse(f.read())

        def visit(node, scope):
            for sub in ast.iter_child_nodes(node):
                if isinstance(sub, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                    is_class = isinstance(sub, ast.ClassDef)
                    inner = scope + [sub.name.upper() if is_class and not sub.name[:1].isupper() else sub.name]
                    if not is_class and any(isinstance(n, ast.Attribute) and n.attr == "_version" for n in ast.walk(sub)):
                        # the outermost function that contains the read names the site (a closure belongs to its function)
                        readers.add(".".join([module] + inner[:2 if inner[0][:1].isupper() else 1]))
                    visit(sub, inner)
                    continue
                if isinstance(sub, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
                    value = getattr(sub, "value", None)
                    new_cache = (isinstance(value, ast.Call) and isinstance(value.func, (ast.Name, ast.Attribute))
                                 and (value.func.id if isinstance(value.func, ast.Name) else value.func.attr) in CACHE_CLASSES)
                    for name in _target_names(sub):
                        if name.endswith("_cache") or new_cache:
                            owner = [s for s in scope if s[:1].isupper()][:1]           # a class attribute or self.<name> of a class
                            sites.add(".".join([module] + owner + [name]))
                if isinstance(sub, ast.Call) and getattr(sub.func, "attr", getattr(sub.func, "id", "")) in ("setattr", "__setattr__"):
                    for a in sub.args:
                        if isinstance(a, ast.Constant) and isinstance(a.value, str) and a.value.endswith("_cache"):
                            sites.add(".".join([module] + [s for s in scope if s[:1].isupper()][:1] + [a.value]))
                visit(sub, scope)
        visit(tree, [])
    return sites, readers


def test_inventory_lists_every_cache():
    sites, readers = _scan()
    assert sites == set(INVENTORY), f"unlisted: {sorted(sites - set(INVENTORY))}; stale: {sorted(set(INVENTORY) - sites)}"
    assert readers == set(VERSION_READERS), f"unlisted: {sorted(readers - set(VERSION_READERS))}; stale: {sorted(set(VERSION_READERS) - readers)}"
    # the kinds in the table are the kinds the cache objects stamp on their pins
    from relation_detr_amd import ms_deform_attn, transformer
    from relation_detr_amd.backbones import resnet
    objects = {"ops._FFN_PACKED": ops._FFN_PACKED, "ops._LINEAR_PACKED": ops._LINEAR_PACKED, "ops._REL_PROJ_F32": ops._REL_PROJ_F32,
               "ms_deform_attn._MERGED_QUERY": ms_deform_attn._MERGED_QUERY, "transformer._VALUE_PROJ": transformer._VALUE_PROJ,
               "backbones.resnet._SCALE_SHIFT": resnet._SCALE_SHIFT}
    for name, cache in objects.items():
        assert isinstance(cache, ops._PackedWeightCache) and cache.kind == INVENTORY[name]["kind"], name


# ------------------------------------------------------------------------------------------------------ mutation matrix
def _get(module, name):
    owner = module
    *path, leaf = name.split(".")
    for part in path:
        owner = getattr(owner, part)
    return owner, leaf, getattr(owner, leaf)


def _put(module, name, tensor):
    owner, leaf, _ = _get(module, name)
    if leaf in owner._parameters:
        owner._parameters[leaf] = tensor
    else:
        owner._buffers[leaf] = tensor


def _changed(t):
    return t.detach().clone() + 1 if not t.is_floating_point() else t.detach().clone() * 1.5 + 0.25


class Case:
    """One cache on CPU tensors: ``module`` owns the sources, ``derive()`` asks the cache, ``recompute()`` is the same arithmetic on
    the current tensors, written out here."""

    def __init__(self, name):
        self.name = name
        torch.manual_seed(0)
        getattr(self, "_" + name)()
        with torch.no_grad():                                    # every source at version >= 1 and non-trivial values
            for s in self.sources:
                t = _get(self.module, s)[2]
                t.add_(torch.arange(t.numel(), dtype=t.dtype).reshape(t.shape) % 5 + 1)

    def _merged(self):
        m = self.module = MultiScaleDeformableAttention(embed_dim=32, num_levels=2, num_heads=4, num_points=2)
        self.sources = ("sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias")
        self.derive = m._merged_query_projection
        self.recompute = lambda: (torch.cat([m.sampling_offsets.weight, m.attention_weights.weight], 0).detach(),
                                  torch.cat([m.sampling_offsets.bias, m.attention_weights.bias], 0).detach())

    def _value(self):
        net = build_relation_transformer(num_classes=3, embed_dim=32, num_heads=4, d_ffn=32, num_levels=2, num_points=2, enc_layers=1,
                                         dec_layers=2, num_queries=4, hybrid_num_proposals=4)
        dec = self.module = net.decoder
        self.sources = tuple(f"layers.{i}.cross_attn.value_proj.{p}" for i in range(2) for p in ("weight", "bias"))
        projs = [layer.cross_attn.value_proj for layer in dec.layers]
        value = torch.linspace(-1, 1, 3 * 32).reshape(1, 3, 32)

        def derive():
            with torch.no_grad():
                return (dec._batched_value_projection(value.to(projs[0].weight.dtype)),)

        def recompute():
            with torch.no_grad():
                w, b = torch.cat([p.weight for p in projs], 0), torch.cat([p.bias for p in projs], 0)
                return (nn.functional.linear(value.to(w.dtype).view(3, 32), w, b).view(1, 3, 64),)
        self.derive, self.recompute = derive, recompute

    def _bn(self):
        m = self.module = FrozenBatchNorm2d(6)
        self.sources = ("weight", "bias", "running_mean", "running_var")
        self.derive = m.scale_shift

        def recompute():
            w, b, rm, rv = (t.detach().float() for t in (m.weight, m.bias, m.running_mean, m.running_var))
            scale = w * (rv + m.eps).rsqrt()
            return scale, b - rm * scale
        self.recompute = recompute

    def _cache_class(self):
        m = self.module = nn.Module()
        m.w, m.b = nn.Parameter(torch.randn(4, 3)), nn.Parameter(torch.randn(4))
        m.register_buffer("s", torch.ones(3))
        self.sources = ("w", "b", "s")
        cache = self.cache = ops._PackedWeightCache()
        self.recompute = lambda: ((m.w.detach() * m.s + m.b.detach()[:, None]).clone(),)
        self.derive = lambda: cache.get((m.w, m.b, m.s), lambda: self.recompute()[0])
        self._wrap = True

    def _host_levels(self):
        m = self.module = nn.Module()
        m.register_buffer("shapes", torch.tensor([[4, 6], [2, 3]]))
        m.register_buffer("start", torch.tensor([0, 24]))
        self.sources = ("shapes", "start")
        as_tensors = lambda levels: tuple(torch.tensor(x) for x in levels)            # noqa: E731
        self.derive = lambda: as_tensors(ops.host_levels(m.shapes, m.start))
        self.recompute = lambda: (m.shapes.clone(), m.start.clone())

    def derived(self):
        out = self.derive()
        return tuple(out) if isinstance(out, (tuple, list)) else (out,)


CASES = ("merged", "value", "bn", "cache_class", "host_levels")
ROUTES = ("inplace", "load_state_dict", "load_state_dict_assign", "data_assign", "to_float64_and_back", "sgd_step", "adamw_step", "stand_in")
# Routes that do not exist for a source: an optimizer steps parameters, never buffers (the batch-norm statistics, the level
# tables, the `s` buffer of the class case); `module.to(float64)` converts floating-point tensors only, so it leaves the int64 level
# tables as they are -- there is no change to detect.
_BUFFERS = {("bn", s) for s in ("weight", "bias", "running_mean", "running_var")} | {("host_levels", "shapes"), ("host_levels", "start"),
                                                                                    ("cache_class", "s")}


def _applies(case, source, route):
    if route in ("sgd_step", "adamw_step"):
        return (case, source) not in _BUFFERS
    if route == "to_float64_and_back":
        return case != "host_levels"
    return True


def _sources_of(case):
    return {"merged": ("sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias"),
            "value": tuple(f"layers.{i}.cross_attn.value_proj.{p}" for i in range(2) for p in ("weight", "bias")),
            "bn": ("weight", "bias", "running_mean", "running_var"), "cache_class": ("w", "b", "s"), "host_levels": ("shapes", "start")}[case]


ROWS = [(c, s, r) for c in CASES for s in _sources_of(c) for r in ROUTES if _applies(c, s, r)]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _assert_fresh(case, before, what, must_change=True):
    got, want = case.derived(), case.recompute()
    assert _same(got, want), f"{case.name}: stale derived data after {what}"
    assert not (must_change and _same(got, before)), f"{case.name}: {what} did not change the derived data (the row proves nothing)"
    return tuple(t.clone() for t in got)


def _apply(case, source, route):
    module = case.module
    owner, leaf, t = _get(module, source)
    if route == "inplace":
        with torch.no_grad():
            t.copy_(_changed(t))
    elif route in ("load_state_dict", "load_state_dict_assign"):
        state = {k: v.detach().clone() for k, v in module.state_dict().items()}
        state[source] = _changed(t)
        module.load_state_dict(state, **({"assign": True} if route.endswith("assign") else {}))
    elif route == "data_assign":
        t.data = _changed(t)
    elif route in ("sgd_step", "adamw_step"):
        from relation_detr_amd.optim import FusedAdamW
        t.grad = torch.ones_like(t)
        opt = torch.optim.SGD([t], lr=0.5) if route == "sgd_step" else FusedAdamW([t], lr=0.5, fused=False)
        opt.step()
        t.grad = None
    elif route == "stand_in":
        # a replaced tensor that reproduces the old key without relying on the allocator: same storage (same data_ptr), changed in
        # place under no_grad until its version equals the old one's -- another object, other content
        assert t._version >= 1
        new = t.data
        new = nn.Parameter(new, requires_grad=t.requires_grad) if isinstance(t, nn.Parameter) else new
        assert new._version == 0 and new.data_ptr() == t.data_ptr() and new is not t
        with torch.no_grad():
            while new._version < t._version:
                new.add_(1)
        assert (new._version, new.data_ptr()) == (t._version, t.data_ptr())
        _put(module, source, new)
    else:
        raise AssertionError(route)


def _check_row(case_name, source, route):
    case = Case(case_name)
    before = tuple(t.clone() for t in case.derived())
    assert _same(before, case.recompute())
    assert _same(case.derived(), before)                         # a second call: the cached data
    if route == "to_float64_and_back":
        case.module.to(torch.float64)
        # another dtype: not the fp32 copy.  (scale_shift is fp32 whatever the buffers are: there the values stay the same, and the
        # perturbation below is what tells a fresh pair from a stale one)
        before = _assert_fresh(case, before, "module.to(float64)", must_change=case_name != "bn")
        assert case_name == "bn" or all(t.dtype == torch.float64 for t in before)
        with torch.no_grad():
            _get(case.module, source)[2].mul_(1.25)
        before = _assert_fresh(case, before, "an in-place op in float64")
        case.module.to(torch.float32)
        before = _assert_fresh(case, before, "module.to(float32) back", must_change=case_name != "bn")
        with torch.no_grad():
            _get(case.module, source)[2].mul_(0.5)
        _assert_fresh(case, before, "an in-place op after the round trip")
        return
    _apply(case, source, route)
    after = _assert_fresh(case, before, f"{route} on {source}")
    # and once more through the same route: the cache must not have latched onto a one-time signal
    if route != "stand_in":
        _apply(case, source, route)
        _assert_fresh(case, after, f"a second {route} on {source}")


@pytest.mark.parametrize("case,source,route", ROWS, ids=[f"{c}-{s}-{r}" for c, s, r in ROWS])
def test_mutation_matrix(case, source, route):
    _check_row(case, source, route)


def test_matrix_covers_every_cache_source_and_route():
    assert {c for c, _, _ in ROWS} == set(CASES)
    for c in CASES:
        assert tuple(Case(c).sources) == _sources_of(c)
        for s in _sources_of(c):
            routes = {r for cc, ss, r in ROWS if (cc, ss) == (c, s)}
            assert {"inplace", "load_state_dict", "load_state_dict_assign", "data_assign", "stand_in"} <= routes, (c, s)
    assert len(ROWS) == sum(_applies(c, s, r) for c in CASES for s in _sources_of(c) for r in ROUTES) >= 110


def test_bn_to_float64_changes_no_value_but_is_still_fresh():
    """scale_shift is fp32 from buffers of any dtype: after module.to(float64) the pair is recomputed from the float64 buffers (the
    same values here, exactly representable), which the matrix row cannot tell from a stale copy -- so the perturbation after it
    is what bites there.  This pins that the row's first step holds for the other cases."""
    bn = FrozenBatchNorm2d(4)
    a = bn.scale_shift()
    bn.to(torch.float64)
    b = bn.scale_shift()
    assert b[0].dtype == torch.float32 and torch.equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------------------------ pins
def _fresh_geometry(monkeypatch):
    monkeypatch.setattr(RelationTransformer, "_geometry_cache", {})


def _check_geometry_pin(monkeypatch):
    from relation_detr_amd import derived
    _fresh_geometry(monkeypatch)
    with derived.recording() as ledger:
        geo = RelationTransformer.level_geometry([(3, 5), (2, 3)], "cpu")
    assert ledger.kinds() == {"level_geometry"}
    refs = [weakref.ref(t) for t in geo.values()]
    want = {k: v.clone() for k, v in geo.items()}
    del geo
    for i in range(20):                                          # 20 further tables, no ledger: the cache clears itself on the way
        RelationTransformer.level_geometry([(7 + i, 2), (1, 1)], "cpu")
        assert len(RelationTransformer._geometry_cache) <= 17
    assert (((3, 5), (2, 3)), "cpu") not in RelationTransformer._geometry_cache     # evicted for eager use, as before
    gc.collect()
    assert all(r() is not None for r in refs), "level_geometry tensors a ledger recorded were freed by the cache's clear()"
    held = {id(t) for t in ledger.tensors()}
    assert all(id(r()) in held for r in refs)
    for r, (k, v) in zip(refs, want.items()):
        assert torch.equal(r(), v), k


def test_geometry_pins_outlive_eviction(monkeypatch):
    _check_geometry_pin(monkeypatch)


def test_geometry_cache_stays_bounded_without_a_ledger(monkeypatch):
    _fresh_geometry(monkeypatch)
    first = weakref.ref(RelationTransformer.level_geometry([(3, 5), (2, 3)], "cpu")["centre"])
    for i in range(40):
        RelationTransformer.level_geometry([(7 + i, 2), (1, 1)], "cpu")
        assert len(RelationTransformer._geometry_cache) <= 17
    gc.collect()
    assert first() is None                                       # nobody pinned it: eviction frees it


def test_planted_missing_geometry_pin_is_caught(monkeypatch):
    from relation_detr_amd import derived
    monkeypatch.setattr(derived, "pin", lambda kind, tensors: None)
    with pytest.raises(AssertionError):
        _check_geometry_pin(monkeypatch)


def test_packed_pin_outlives_a_rebuild_for_eager_use():
    """A source changes version while a ledger holds the old copy: the eager path builds a NEW copy (it must not write into a
    buffer a graph may be reading on another stream), the ledger keeps the old one alive at its address."""
    from relation_detr_amd import derived
    cache = derived.DerivedCache(kind="t")
    w = nn.Parameter(torch.arange(6.0).reshape(2, 3))
    build = lambda: w.detach() * 2                               # noqa: E731
    fill = lambda d, s: d.copy_(s.detach() * 2)                  # noqa: E731
    with derived.recording() as ledger:
        old = cache.get((w,), build, fill)
        assert cache.get((w,), build, fill) is old and len(ledger.pins) == 1
    ref, address = weakref.ref(old), old.data_ptr()
    del old
    with torch.no_grad():
        w.add_(1)
    new = cache.get((w,), build, fill)
    assert new is not ref() and torch.equal(new, w.detach() * 2)
    for i in range(70):                                          # past the prune interval
        t = torch.full((2,), float(i))
        cache.get((t,), lambda: t * 2)
    gc.collect()
    assert ref() is not None and ref().data_ptr() == address and ledger.pins[0].derived is ref()
    assert ledger.refresh() == 1 and torch.equal(ref(), w.detach() * 2) and ref().data_ptr() == address
    del ledger
    gc.collect()
    assert ref() is None                                         # the pin was the last reference


# ------------------------------------------------------------------------------------------------------ replay decision
def _decision_fixture():
    from relation_detr_amd import derived
    m = nn.Module()
    m.w, m.b = nn.Parameter(torch.arange(12.0).reshape(4, 3)), nn.Parameter(torch.ones(4))
    cache = derived.DerivedCache(kind="affine")
    fill = lambda d, w, b: d.copy_(w.detach() + b.detach()[:, None])         # noqa: E731  (takes the sources: holds none)
    with derived.recording() as ledger:
        d = cache.get((m.w, m.b), lambda: m.w.detach() + m.b.detach()[:, None], fill)
    ledger.name_sources([m])
    return derived, m, ledger, d


def _actions(derived, ledger, **kw):
    return [a for _, a in derived.replay_decision(ledger, **kw)]


def test_replay_decision_refreshes_in_place():
    derived, m, ledger, d = _decision_fixture()
    address = d.data_ptr()
    # unchanged: the copy is current, nothing to do; a forced refresh (after a `.data` write) is "refresh in place" for it too
    assert _actions(derived, ledger) == [derived.KEEP] and ledger.refresh() == 0
    assert _actions(derived, ledger, force=True) == [derived.REFRESH] == ["refresh in place"]
    # a version bump at the same address
    with torch.no_grad():
        m.b.mul_(3)
    assert _actions(derived, ledger) == ["refresh in place"]
    assert ledger.refresh() == 1 and d.data_ptr() == address and torch.equal(d, m.w.detach() + m.b.detach()[:, None])
    assert _actions(derived, ledger) == [derived.KEEP]
    # load_state_dict: copies into the parameters where they stand
    m.load_state_dict({"w": torch.full((4, 3), 2.0), "b": torch.full((4,), -1.0)})
    assert _actions(derived, ledger) == ["refresh in place"]
    assert ledger.refresh() == 1 and d.data_ptr() == address and torch.equal(d, torch.ones(4, 3))
    # an unsignalled write: invisible (documented), until forced
    m.w.data.mul_(2)
    assert _actions(derived, ledger) == [derived.KEEP] and torch.equal(d, torch.ones(4, 3))
    assert ledger.refresh(force=True) == 1 and torch.equal(d, torch.full((4, 3), 3.0)) and d.data_ptr() == address


def test_replay_decision_raises_for_moved_retyped_and_dead_sources():
    derived, m, ledger, d = _decision_fixture()
    keep = d.clone()
    m.b.data = torch.zeros(4)                                    # moved
    with pytest.raises(_lib.RdetrError, match=r"`b` moved to another address"):
        derived.replay_decision(ledger)
    with pytest.raises(_lib.RdetrError, match="`b`"):
        ledger.refresh()
    assert torch.equal(d, keep)                                  # nothing was rebuilt
    derived, m, ledger, d = _decision_fixture()
    m.to(torch.float64)                                          # changed dtype (and address)
    with pytest.raises(_lib.RdetrError, match=r"`w` (moved|changed dtype)"):
        derived.replay_decision(ledger)
    derived, m, ledger, d = _decision_fixture()
    m.load_state_dict({"w": torch.zeros(4, 3), "b": torch.zeros(4)}, assign=True)        # new objects; the old ones die
    gc.collect()
    with pytest.raises(_lib.RdetrError, match="no longer exists"):
        derived.replay_decision(ledger)
    with pytest.raises(_lib.RdetrError, match="no longer exists"):
        ledger.refresh(force=True)


def _check_refresh_in_place():
    """What a graph's refresh must do to a merged projection: the pinned buffers, at their addresses, hold the current sources."""
    from relation_detr_amd import derived
    m = MultiScaleDeformableAttention(embed_dim=32, num_levels=2, num_heads=4, num_points=2)
    with derived.recording() as ledger:
        w, b = m._merged_query_projection()
    addresses = (w.data_ptr(), b.data_ptr())
    with torch.no_grad():
        m.attention_weights.bias.add_(2)
        m.sampling_offsets.weight.add_(1)
    assert ledger.refresh() == 1
    assert (w.data_ptr(), b.data_ptr()) == addresses
    assert torch.equal(w, torch.cat([m.sampling_offsets.weight, m.attention_weights.weight], 0))
    assert torch.equal(b, torch.cat([m.sampling_offsets.bias, m.attention_weights.bias], 0))


def test_refresh_rebuilds_into_the_pinned_buffers():
    _check_refresh_in_place()


def test_planted_rebuild_that_returns_the_old_copy_is_caught(monkeypatch):
    from relation_detr_amd import ms_deform_attn
    monkeypatch.setattr(ms_deform_attn, "_fill_merged", lambda merged, *sources: merged)
    with pytest.raises(AssertionError):
        _check_refresh_in_place()


def test_planted_key_without_the_bias_address_is_caught(monkeypatch):
    """The hole of the keys this file was written against: a 1-d source's address left out of the key."""
    from relation_detr_amd import derived
    real = derived.stamp
    monkeypatch.setattr(derived, "stamp", lambda t: real(t) if t.dim() != 1 else (t._version, 0, t.shape, t.dtype, t.device))
    _check_row("merged", "sampling_offsets.weight", "data_assign")           # weights are still seen
    for case, source in (("merged", "attention_weights.bias"), ("value", "layers.1.cross_attn.value_proj.bias"), ("bn", "running_var")):
        with pytest.raises(AssertionError, match="stale derived data"):
            _check_row(case, source, "data_assign")


def test_drop_all_empties_every_cache(monkeypatch):
    from relation_detr_amd import derived
    _fresh_geometry(monkeypatch)
    derived.on_drop(RelationTransformer._geometry_cache.clear)
    case = Case("merged")
    before = case.derived()
    case.module.sampling_offsets.bias.data.mul_(1.5)             # unsignalled: the cache cannot see it
    assert _same(case.derived(), before) and not _same(before, case.recompute())
    bn = Case("bn")
    bn.derived()
    RelationTransformer.level_geometry([(2, 2)], "cpu")
    ops.host_levels(torch.tensor([[2, 2]]), torch.tensor([0]))
    derived.drop_all()
    assert len(ops._LINEAR_PACKED) == len(ops._FFN_PACKED) == len(ops._REL_PROJ_F32) == 0
    assert not RelationTransformer._geometry_cache and not ops._shape_cache and not ops._window_ok_cache and not ops._host_array_cache
    assert _same(case.derived(), case.recompute())
    derived._droppers.pop()


def test_no_fill_closes_over_a_variable():
    """A ledger keeps each copy's ``fill``; one that closed over a variable of the call that made it (a weight, a module) would keep a
    replaced parameter alive, and the replay decision would never learn that it died.  From the symbol tables of the package: every
    function whose name starts with ``fill`` or ``_fill`` has no free variable."""
    import symtable
    found = []

    def walk(table, module):
        for child in table.get_children():
            if child.get_type() == "function" and child.get_name().lstrip("_").startswith("fill"):
                found.append(f"{module}.{child.get_name()}")
                assert not child.get_frees(), f"{module}.{child.get_name()} (line {child.get_lineno()}) closes over {child.get_frees()}"
            walk(child, module)
    for module, path in _package_files():
        with open(path) as f:
            walk(symtable.symtable(f.read(), path, "exec"), module)
    assert len([n for n in found if n.startswith("ops.")]) >= 7 and "ms_deform_attn._fill_merged" in found, found
