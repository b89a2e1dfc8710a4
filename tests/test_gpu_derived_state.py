"""Weights change under cached copies and under captured graphs (relation_detr_amd/derived.py).

The network and inputs are those of test_gpu_glue::test_graph_replay_matches_eager (B = 2), loaded with helpers.synthetic_state_dict so
that no source is zero.  The oracle is always an eager forward of a net of NEW module objects (a deep copy of a template that never
ran: module-level caches are keyed by tensor object, so it shares no entry) loaded with ``net.state_dict()``; the full per-layer
``classes`` / ``coords`` stacks are compared bit for bit.  Before every replay the host asserts that every tensor the graph pinned is
alive at its captured address, so a wrong fix fails before anything is launched.

Kinds per configuration (what the code routes, read from transformer.py / ms_deform_attn.py / self_attn.py): bf16 default uses the
linear packs, the relation projection's fp32 copy, the merged query projection and the level tables; ``decoder_value_batched`` adds
the batched value projection; fp32 uses the merged projection and the level tables only (the packs, the batched value projection and
the in-kernel relation bias are bf16 routes).  The fused FFN -- and ``linear_k256`` / ``ffn_ln`` with it -- takes inputs of at least
transformer._K256_MIN_ROWS = 16384 rows; this network has B * S = 2 * 2975, so its FFN pack is exercised on a tall input of its own
(test_ffn_pack_follows_its_weights).  The folded batch-norm pair belongs to the backbone, which this network does not have: its rows
are in tests/test_derived_state_host.py."""
import copy
import functools
import weakref

import pytest
import torch

import dirty
import shadow
from helpers import synthetic_state_dict
from test_derived_state_host import INVENTORY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(40, 56), (20, 28), (10, 14), (5, 7)]
B, L = 2, len(SHAPES)
OPT_IN = dict(decoder_value_batched=True, linear_k256=True, ffn_ln=True)
BF16_KINDS = {"linear_packed", "rel_proj_f32", "merged_query_projection", "level_geometry"}
CONFIGS = {
    "bf16": (torch.bfloat16, {}, BF16_KINDS),
    "bf16-optin": (torch.bfloat16, OPT_IN, BF16_KINDS | {"value_projection_batched"}),
    "fp32": (torch.float32, {}, {"merged_query_projection", "level_geometry"}),
}


@functools.lru_cache(maxsize=None)
def _template(config):
    """A net of the configuration on the device that never runs a forward: `_fresh` deep-copies it."""
    from relation_detr_amd import options
    from relation_detr_amd.transformer import build_relation_transformer
    dtype, opts, _ = CONFIGS[config]
    with options.override(**opts):
        net = build_relation_transformer(num_classes=17, d_ffn=128, enc_layers=2, dec_layers=2, num_queries=50, hybrid_num_proposals=60)
    net.load_state_dict(synthetic_state_dict(net.state_dict()))
    return net.eval().to(DEV).to(dtype)


def _fresh(config, state=None):
    net = copy.deepcopy(_template(config))
    if state is not None:
        net.load_state_dict(state)
    return net


@functools.lru_cache(maxsize=None)
def _inputs(dtype):
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn(B, 256, h, w, generator=g).to(DEV, dtype) for h, w in SHAPES]
    pos = [torch.randn(B, 256, h, w, generator=g).to(DEV, dtype) for h, w in SHAPES]
    masks = []
    for h, w in SHAPES:
        m = torch.zeros(B, h, w, dtype=torch.bool)
        m[1, :, int(w * 0.8):] = True                           # image 1 is right-padded
        masks.append(m.to(DEV))
    return (*feats, *masks, *pos)


def _forward_of(net):
    @torch.no_grad()
    def forward(*t):
        classes, coords = net(list(t[:L]), list(t[L:2 * L]), list(t[2 * L:3 * L]))[:2]
        # every layer's output, batch first (ImageGroups concatenates along dim 0)
        return torch.stack(list(classes)).transpose(0, 1).contiguous(), torch.stack(list(coords)).transpose(0, 1).contiguous()
    return forward


def _eager(net, inputs, groups=1):
    from relation_detr_amd.graph import ImageGroups
    fwd = _forward_of(net)
    out = (ImageGroups(fwd, groups, device=DEV) if groups > 1 else fwd)(*inputs)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def _want(config, net, inputs, groups=1):
    return _eager(_fresh(config, net.state_dict()), inputs, groups)


def _equal(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def _new_values(t, k=0):
    """Other values of the same scale, deterministic, different for every k."""
    idx = torch.arange(t.numel(), device=t.device, dtype=torch.float32).reshape(t.shape)
    f = t.detach().float()
    return (f * 0.75 + (f.abs().mean() + 1e-3) * 0.5 * torch.cos(idx * 0.61 + k)).to(t.dtype)


def _other_state(net, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (v.float() * 0.9 + v.float().abs().mean() * 0.3 * torch.randn(v.shape, generator=g).to(v.device)).to(v.dtype)
            if v.is_floating_point() else v.clone() for k, v in net.state_dict().items()}


def _kinds(ledger):
    """Cache kinds of a ledger's pins ("linear_packed.k_halves" is a use of the cache "linear_packed")."""
    return {k.split(".")[0] for k in ledger.kinds()}


def _snapshot(ledger):
    return [(weakref.ref(t), t.data_ptr()) for t in ledger.tensors()]


def _assert_pins(snapshot):
    """Host only: every tensor the graph read from a cache is alive at its captured address."""
    assert snapshot
    for ref, address in snapshot:
        t = ref()
        assert t is not None, "a tensor a live graph reads was freed"
        assert t.data_ptr() == address, "a tensor a live graph reads moved"


def _churn(ledger):
    """Free and re-allocate 64 blocks of each float-valued pin's size, filled with 0x42 bytes: a copy that was freed under a graph
    would now hold 48.5 (bf16) / 4.9e1 (fp32), far outside every weight."""
    poison = dirty.Poison(0x42)
    for t in ledger.tensors():
        if t.is_floating_point():
            blocks = [poison.fill(torch.empty(t.numel(), dtype=t.dtype, device=t.device)) for _ in range(64)]
            del blocks
    torch.cuda.synchronize()


def _graph(net, inputs, groups=1, **kw):
    from relation_detr_amd.graph import GraphedCall, ImageGroups
    fwd = _forward_of(net)
    run = GraphedCall(ImageGroups(fwd, groups, device=DEV) if groups > 1 else fwd, [t.clone() for t in inputs], **kw)
    return run, _snapshot(run.ledger)


def _replay(run, snapshot, inputs):
    _assert_pins(snapshot)
    out = run(*inputs)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def _named(net, tensor):
    return next(n for n, p in list(net.named_parameters()) + list(net.named_buffers()) if p is tensor)


SATURATED = ("bbox_head", "position_relation_embedding")


def _source(ledger, kinds, dim, net):
    """The first source with ``dim`` dimensions of a pin whose kind starts with one of ``kinds``, the box heads left out: under the
    synthetic weights their outputs saturate (see test_eager_forward_follows_every_source), so a change there shows in no output."""
    for pin in ledger.pins:
        if pin.kind.startswith(kinds):
            for ref in pin.sources:
                if ref() is not None and ref().dim() == dim and not any(n in _named(net, ref()) for n in SATURATED):
                    return ref()
    raise AssertionError(f"no {dim}-d source of {kinds} in the ledger")


def _derived_bits(ledger):
    return [t.clone() for t in ledger.tensors()]


def _same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ G1, eager
@pytest.mark.parametrize("route", ["inplace", "data_assign"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_eager_forward_follows_every_source(config, route, monkeypatch):
    """Every source the forward's ledger lists, one at a time: the outputs AND the derived copies the forward used are, bit for bit,
    those of a fresh net with the same state, and both differ from what they were before the change.
    One exception to "the output differs", by the fixture and not by the code: helpers.synthetic_state_dict gives the three-layer
    box heads coherent sine weights whose outputs run far into the sigmoid's flat ends, where the refinement's eps clamp (1e-3)
    pins every box at 0.001 / 0.999 -- a changed box-head weight then changes no output bit.  With every box at the clamp all pairs
    of boxes have the same relation features, so the relation projection's bias is one constant per head over all keys, which the
    softmax cancels: its sources cannot show in an output either.  For those sources (names holding one of SATURATED) the derived
    copy itself carries the row: it must differ from its previous bits and equal the fresh net's."""
    from relation_detr_amd import derived
    dtype, _, kinds = CONFIGS[config]
    inputs = _inputs(dtype)
    net = _fresh(config)

    def forward(n):
        with derived.recording() as ledger:
            out = _eager(n, inputs)
        return out, _derived_bits(ledger), ledger
    previous, previous_bits, ledger = forward(net)
    assert _kinds(ledger) <= {row["kind"] for row in INVENTORY.values()}
    assert _kinds(ledger) == kinds, f"the forward used {sorted(_kinds(ledger))}, the configuration is expected to use {sorted(kinds)}"
    want, want_bits, _ = forward(_fresh(config, net.state_dict()))
    assert _equal(previous, want) and _same_bits(previous_bits, want_bits)
    sources = ledger.sources()                                   # every source tensor of every copy the forward used
    assert len(sources) >= (20 if dtype == torch.bfloat16 else 8) and any(s.dim() == 1 for s in sources)
    for k, source in enumerate(sources):
        name = _named(net, source)
        with torch.no_grad():
            if route == "inplace":
                source.copy_(_new_values(source, k))
            else:
                source.data = _new_values(source, k)
        got, got_bits, _ = forward(net)
        want, want_bits, _ = forward(_fresh(config, net.state_dict()))
        assert _equal(got, want), f"stale derived data after {route} on {name}: the outputs are not the fresh net's"
        assert _same_bits(got_bits, want_bits), f"stale derived data after {route} on {name}: the copies are not the fresh net's"
        assert not _same_bits(got_bits, previous_bits), f"{route} on {name} changed no derived copy"
        assert any(n in name for n in SATURATED) or not _equal(got, previous), f"{route} on {name} changed no output: the source is not used"
        previous, previous_bits = got, got_bits
    sh = shadow.Shadow(monkeypatch)                              # float64 check of the operands the entries were handed
    _eager(net, inputs)
    sh.assert_ok()


# ----------------------------------------------------------------------------------------------------------- G2, replay
PACKED = ("linear_packed",)


def _changes(net, ledger, weight_kinds=PACKED):
    """(label, apply) in the order of the issue; the sources come from the graph's own ledger.  fp32 has no packed copy: there the
    merged projection's weight stands in for the packed source."""
    packed = _source(ledger, weight_kinds, 2, net)
    bias = _source(ledger, ("merged_query_projection",), 1, net)

    def load():
        net.load_state_dict(_other_state(net, 11))

    def inplace(t, k):
        def go():
            with torch.no_grad():
                t.copy_(_new_values(t, k))
        return go

    def step():
        params = [p for p in net.parameters()]
        for i, p in enumerate(params):
            p.grad = _new_values(p, 100 + i)
        torch.optim.SGD(params, lr=0.05).step()
        for p in params:
            p.grad = None
    return [("load_state_dict", load), (f"in-place on {_named(net, packed)}", inplace(packed, 1)),
            (f"in-place on {_named(net, bias)}", inplace(bias, 2)), ("torch.optim.SGD step", step)]


@pytest.mark.parametrize("eager_between", [False, True], ids=["replay-first", "eager-forward-between"])
@pytest.mark.parametrize("config", ["bf16", "bf16-optin", "fp32"])
def test_replay_follows_weight_changes(config, eager_between):
    dtype, _, kinds = CONFIGS[config]
    inputs = _inputs(dtype)
    net = _fresh(config)
    run, pins = _graph(net, inputs)
    assert _kinds(run.ledger) == kinds
    assert _equal(_replay(run, pins, inputs), _want(config, net, inputs))
    previous = None
    for label, change in _changes(net, run.ledger, PACKED if dtype == torch.bfloat16 else ("merged_query_projection",)):
        change()
        if eager_between:
            _eager(net, inputs)                                  # the caches rebuild for eager use and drop their old copies
            _churn(run.ledger)
        got = _replay(run, pins, inputs)
        assert _equal(got, _want(config, net, inputs)), f"replay after {label} is not the eager forward of a fresh net"
        assert previous is None or not _equal(got, previous), label
        previous = got


def test_replay_through_image_groups_follows_weight_changes():
    config = "bf16"
    inputs = _inputs(torch.bfloat16)
    net = _fresh(config)
    run, pins = _graph(net, inputs, groups=2)
    assert _equal(_replay(run, pins, inputs), _want(config, net, inputs, groups=2))
    for label, change in _changes(net, run.ledger):
        change()
        assert _equal(_replay(run, pins, inputs), _want(config, net, inputs, groups=2)), label


def test_replay_refuses_moved_weights_before_launching(monkeypatch):
    from relation_detr_amd import _lib
    config = "bf16"
    inputs = _inputs(torch.bfloat16)
    net = _fresh(config)
    run, pins = _graph(net, inputs)
    want = _replay(run, pins, inputs)
    packed = _source(run.ledger, PACKED, 2, net)
    name = _named(net, packed)
    sh = shadow.Shadow(monkeypatch, check=False)                 # counting tripwires on every launching symbol, nothing else
    old = packed.data
    packed.data = old.clone()                                    # same values, another address: the graph reads the old one
    _assert_pins(pins)
    before = sum(sh.launches.values())
    with pytest.raises(_lib.RdetrError, match=name.replace(".", r"\.") + ".*moved"):
        run(*inputs)
    assert sum(sh.launches.values()) == before
    packed.data = old                                            # back where it was captured: replays again
    assert _equal(_replay(run, pins, inputs), want)
    net.to(torch.float32)
    _assert_pins(pins)
    before = sum(sh.launches.values())
    with pytest.raises(_lib.RdetrError, match="moved|changed dtype"):
        run(*inputs)
    assert sum(sh.launches.values()) == before


def test_check_weights_false_keeps_the_unchecked_replay():
    """``check_weights=False``: no walk, so a changed weight is not noticed -- the packed copy stays as captured while the library
    GEMMs read the new weights -- until the caller refreshes by hand.  Only live (pinned) memory is read."""
    config = "bf16"
    inputs = _inputs(torch.bfloat16)
    net = _fresh(config)
    run, pins = _graph(net, inputs, check_weights=False)
    packed = _source(run.ledger, PACKED, 2, net)
    with torch.no_grad():
        packed.copy_(_new_values(packed, 3))
    want = _want(config, net, inputs)
    assert not _equal(_replay(run, pins, inputs), want)
    assert run.refresh_weights() == len([p for p in run.ledger.pins if p.sources])
    assert _equal(_replay(run, pins, inputs), want)


def test_ffn_pack_follows_its_weights():
    """The (w1, w2) pack of ffn_k256 at the smallest height the stack sends it (16384 rows): eager and replayed, after an in-place
    change of either weight, the bits are those of the same call on NEW parameter objects with the same values."""
    from relation_detr_amd import ops
    from relation_detr_amd.graph import GraphedCall
    rows, F = 16384, 128
    idx = lambda *shape: torch.arange(int(torch.tensor(shape).prod()), device=DEV, dtype=torch.float32).reshape(shape)   # noqa: E731
    x = torch.sin(idx(rows, 256) * 0.013).to(torch.bfloat16)
    make = lambda shape, k, s: torch.nn.Parameter((torch.sin(idx(*shape) * 0.7071 + k) * s).to(torch.bfloat16))            # noqa: E731
    w1, b1, w2, b2 = make((F, 256), 0, 0.1), make((F,), 1, 0.05), make((256, F), 2, 0.15), make((256,), 3, 0.05)

    @torch.no_grad()
    def call(*p):
        return ops.ffn_k256(x, *p)

    def want():
        out = call(*[torch.nn.Parameter(p.detach().clone()) for p in (w1, b1, w2, b2)])
        torch.cuda.synchronize()
        return out.clone()
    run = GraphedCall(lambda t: call(w1, b1, w2, b2), [x])
    pins = _snapshot(run.ledger)
    assert _kinds(run.ledger) == {"ffn_packed"} and len(run.ledger.sources()) == 2
    previous = want()
    _assert_pins(pins)
    assert torch.equal(run(x).clone(), previous)
    for k, (t, between) in enumerate([(w1, False), (w2, True), (w1, True), (w2, False)]):
        with torch.no_grad():
            t.copy_(_new_values(t, k))
        now = want()
        assert not torch.equal(now, previous)
        if between:
            assert torch.equal(call(w1, b1, w2, b2), now)
            _churn(run.ledger)
        _assert_pins(pins)
        got = run(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, now), k
        assert torch.equal(call(w1, b1, w2, b2), now)
        previous = now


# --------------------------------------------------------------------------------------------------------- G3, geometry
def test_graph_keeps_its_level_tables_through_eviction():
    from relation_detr_amd.transformer import RelationTransformer
    config = "bf16"
    inputs = _inputs(torch.bfloat16)
    net = _fresh(config)
    want = _eager(net, inputs)
    run, pins = _graph(net, inputs)
    assert "level_geometry" in _kinds(run.ledger)
    for i in range(17):                                          # host calls only: 17 other pyramids evict ours from the cache
        RelationTransformer.level_geometry([(3 + i, 2), (2, 1), (1, 1), (1, 1)], DEV)
    assert (tuple(SHAPES), str(torch.device(DEV))) not in RelationTransformer._geometry_cache and \
           (tuple(SHAPES), DEV) not in RelationTransformer._geometry_cache
    _churn(run.ledger)
    assert _equal(_replay(run, pins, inputs), want)


# ------------------------------------------------------------------------------------------------ G4, unsignalled write
def test_data_write_needs_the_two_documented_calls():
    from relation_detr_amd import derived
    config = "bf16"
    inputs = _inputs(torch.bfloat16)
    net = _fresh(config)
    run, pins = _graph(net, inputs)
    packed = _source(run.ledger, PACKED, 2, net)
    version = packed._version
    packed.data.mul_(1.5)
    assert packed._version == version                            # torch gives no signal
    want = _want(config, net, inputs)
    assert not _equal(_eager(net, inputs), want)                 # documented: invisible to the caches ...
    derived.drop_all()
    assert _equal(_eager(net, inputs), want)                     # ... until every eager entry is dropped
    assert not _equal(_replay(run, pins, inputs), want)          # the graph still reads the copy it pinned ...
    assert run.refresh_weights() >= 1
    assert _equal(_replay(run, pins, inputs), want)              # ... until it is told to rebuild them


# ----------------------------------------------------------------------------------- G5, train in fp32, serve in bf16
def test_bf16_serving_copy_follows_a_fused_training_step():
    """The bf16 sibling of test_gpu_optim::test_step_invalidates_the_weight_caches: an fp32 head takes one fused AdamW step, a
    persistent bf16 copy of its transformer is refreshed with load_state_dict, and both its eager forward and its graph must be
    the forward of a bf16 net built fresh from the same state."""
    from relation_detr_amd.optim import FusedAdamW, relation_param_groups, train_step
    from test_denoising_host import head_inputs, tiny_head
    head = tiny_head(DEV, True)
    (feats, masks, pos), targets = head_inputs(DEV)
    template = copy.deepcopy(head.transformer).to(torch.bfloat16).eval()         # never runs: the fresh nets are copies of it
    serving = copy.deepcopy(template)
    inputs = [*[f.to(torch.bfloat16) for f in feats], *masks, *[p.to(torch.bfloat16) for p in pos]]
    levels = len(feats)

    def forward_of(net):
        @torch.no_grad()
        def forward(*t):
            classes, coords = net(list(t[:levels]), list(t[levels:2 * levels]), list(t[2 * levels:3 * levels]))[:2]
            return torch.stack(list(classes)), torch.stack(list(coords))
        return forward

    def eager(net):
        out = forward_of(net)(*inputs)
        torch.cuda.synchronize()
        return tuple(t.clone() for t in out)
    from relation_detr_amd.graph import GraphedCall
    run = GraphedCall(forward_of(serving), [t.clone() for t in inputs])
    pins = _snapshot(run.ledger)
    assert {"linear_packed", "merged_query_projection"} <= _kinds(run.ledger)      # a bf16 cache is in play
    before = eager(serving)
    opt = FusedAdamW(relation_param_groups(head, 1e-3), lr=1e-3, weight_decay=1e-4, fused=True)
    head.train()
    train_step(head, opt, feats, masks, pos, targets)
    serving.load_state_dict(head.transformer.state_dict())
    fresh = copy.deepcopy(template)
    fresh.load_state_dict(head.transformer.state_dict())
    want = eager(fresh)
    assert not _equal(want, before)
    _assert_pins(pins)
    replay = tuple(t.clone() for t in run(*inputs))
    torch.cuda.synchronize()
    assert _equal(replay, want), "the graph of the serving copy did not follow load_state_dict"
    assert _equal(eager(serving), want), "the eager forward of the serving copy did not follow load_state_dict"
