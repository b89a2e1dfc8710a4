"""GPU checks of the optimizer step (csrc/optim.hip, relation_detr_amd/optim.py): global-norm clip and AdamW on the fused route.

The checker is the torch route's (``FusedAdamW(fused=False)``) single step in float64, started from the kernel's own state before
that step; ``e32`` is the error of the same route in fp32 against it.  All bounds are elementwise, with gc = |g * coef| of the checker:
    exp_avg      max(4 e32, 2^-20 max(|m_old|, gc))
    exp_avg_sq   max(4 e32, 2^-20 max(v_old, gc^2))
    param        max(4 e32, 2^-20 (|p_old| + step_size (|m_old| + gc) / denom64))
    total norm   max(4 e32, 2^-20 |checker|)
The kernel computes in fp32 in the fp32 route's operation order; 2^-20 = 8 fp32 ulps of the scale covers the elements where the
fp32 route happens to round to the checker.  The update's own magnitude belongs in the parameter's scale: a parameter that an update
carries through zero would otherwise be held to its own tiny magnitude.  A scale of 0 demands an exact 0."""
import copy

import pytest
import torch

from helpers import snapshot, torch_route_step
from relation_detr_amd.optim import CHUNK, FusedAdamW, relation_param_groups, step_scalars, train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
FLOOR = 2.0 ** -20
MAX_NORM = 0.1
SIZES = (1, 3, 4, 5, 91, 256, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)


# ------------------------------------------------------------------------------------------------------------------------ checker
class Worst:
    """The worst fraction of its bound per compared quantity; 0 / 0 counts as 0, anything / 0 as inf."""

    def __init__(self):
        self.worst = {}

    def add(self, what, got, checker, fp32, scale):
        e32 = (fp32.to(F64) - checker).abs()
        bound = torch.maximum(4 * e32, FLOOR * scale)
        err = (got.to(F64) - checker).abs()
        frac = torch.where(err == 0, torch.zeros_like(err), err / bound).max().reshape(1)
        self.worst[what] = torch.maximum(self.worst[what], frac) if what in self.worst else frac

    def report(self, title):
        worst = {k: v.item() for k, v in self.worst.items()}
        print(f"{title}: worst fraction of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        for k, v in worst.items():
            assert v <= 1.0, (title, k, v)


def check_step(title, opt, max_norm=MAX_NORM, clip=True):
    """Run one clip + step of ``opt`` on the fused route and compare everything it wrote with the checker."""
    rows = snapshot(opt)
    moment_version = lambda p: opt.state[p]["exp_avg"]._version if opt.state.get(p) else 0
    versions = [(p._version, moment_version(p)) for g in opt.param_groups for p in g["params"]]
    norm = opt.clip_grad_norm_(max_norm) if clip else None
    assert (opt.clip_coef is not None) == clip
    coef = opt.clip_coef.clone() if clip else None
    opt.step()
    assert opt.clip_coef is None                                                # one clip arms one step
    norm64, want = torch_route_step(opt, rows, max_norm if clip else None, F64)
    norm32, fp32 = torch_route_step(opt, rows, max_norm if clip else None, F32)
    worst = Worst()
    if clip:
        assert norm.ndim == 0 and norm.dtype == F32 and norm.device == opt.param_groups[0]["params"][0].device
        worst.add("norm", norm, norm64, norm32, norm64.abs())
        c64 = (max_norm / (norm64 + 1e-6)).clamp(max=1.0)
        worst.add("coef", coef, c64, (max_norm / (norm32 + 1e-6)).clamp(max=1.0), c64)
    i = 0
    for group in opt.param_groups:
        beta1, beta2 = group["betas"]
        for p in group["params"]:
            row, (p64, m64, v64, g64), (p32, m32, v32, _) = rows[i], want[i], fp32[i]
            state = opt.state.get(p) or {}
            if row["g"] is None:                                                # untouched: bits, step and version
                assert torch.equal(p, row["p"]) and p._version == versions[i][0], i
                assert state.get("step", 0.0) == row["step"] and (not state or torch.equal(state["exp_avg"], row["m"])), i
                assert not state or (state["exp_avg"]._version == versions[i][1] and torch.equal(state["exp_avg_sq"], row["v"])), i
            else:
                assert p._version > versions[i][0] and float(state["step"]) == row["step"] + 1, i
                assert state["exp_avg"]._version > versions[i][1] and state["exp_avg_sq"]._version > 0, i
                assert torch.equal(p.grad, row["g"]), i                         # the gradient is only read: it keeps its unclipped value
                scalars = step_scalars(group["lr"], beta1, beta2, group["eps"], group["weight_decay"], row["step"] + 1)
                step_size, bias2_sqrt = scalars[4], scalars[5]
                m_old = torch.zeros_like(p64) if row["m"] is None else row["m"].to(F64).abs()
                v_old = torch.zeros_like(p64) if row["v"] is None else row["v"].to(F64)
                gc = g64.abs()
                denom = v64.sqrt() / bias2_sqrt + group["eps"]
                worst.add("exp_avg", state["exp_avg"], m64, m32, torch.maximum(m_old, gc))
                worst.add("exp_avg_sq", state["exp_avg_sq"], v64, v32, torch.maximum(v_old, gc * gc))
                worst.add("param", p.detach(), p64, p32, row["p"].to(F64).abs() + step_size * (m_old + gc) / denom)
            i += 1
    worst.report(title)
    return norm


# ------------------------------------------------------------------------------------------------------------------------ inputs
def boundary_params(seed=0):
    """The boundary sizes, a parameter that is a view at element offset 1 of a larger buffer (4-byte aligned only), a 2-D one, an
    all-zero one, one that never has a gradient and a frozen one, in three groups."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.randn(*s, generator=g).to(DEV)
    params = [torch.nn.Parameter(rand(n)) for n in SIZES]
    params.append(torch.nn.Parameter(rand(CHUNK + 6)[1:]))                      # [10] offset view
    params.append(torch.nn.Parameter(rand(8, 6)))                               # [11] gets a non-contiguous gradient
    params.append(torch.nn.Parameter(torch.zeros(300, device=DEV)))             # [12] zero parameter, zero gradient
    params.append(torch.nn.Parameter(rand(77)))                                 # [13] never has a gradient
    params.append(torch.nn.Parameter(rand(50), requires_grad=False))            # [14] frozen
    params.append(torch.nn.Parameter(rand(1000)))                               # [15] its gradient is an offset view
    params.append(torch.nn.Parameter(rand(129)))                                # [16] no gradient on odd steps
    assert params[10].data_ptr() % 16 == 4 and params[10].is_contiguous()
    groups = [{"params": params[:6] + params[12:]}, {"params": params[6:9], "weight_decay": 0.0}, {"params": params[9:12], "lr": 3e-4}]
    return params, groups


def set_boundary_grads(params, step, seed=0):
    g = torch.Generator().manual_seed(7919 * seed + step)
    scale = (1.0, 1e-4, 1e-2, 1e-5, 1.0)[step]                                  # clipped, not, clipped, not, clipped
    rand = lambda *s: (torch.randn(*s, generator=g) * scale).to(DEV)
    for i, p in enumerate(params):
        if i in (13, 14) or (i == 16 and step % 2 == 1):
            p.grad = None
        elif i == 11:
            p.grad = rand(6, 8).t()
        elif i == 12:
            p.grad = torch.zeros_like(p)
        elif i == 15:
            p.grad = rand(p.numel() + 1)[1:]
        else:
            p.grad = rand(*p.shape)
            if i == 4 and step == 0:
                p.grad[::2] = 0                                                 # zero gradients on a non-zero parameter
    assert not params[11].grad.is_contiguous() and params[15].grad.data_ptr() % 16 == 4


def boundary_run(steps=5, seed=0):
    params, groups = boundary_params(seed)
    opt = FusedAdamW(groups, lr=1e-3, weight_decay=1e-2, fused=True)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.1, total_iters=4)
    return params, opt, sched


# ------------------------------------------------------------------------------------------------------------------------ tests
def test_boundary_set_five_steps_under_linear_lr():
    params, opt, sched = boundary_run()
    assert opt._on_fused_route()
    norms = []
    for step in range(5):
        set_boundary_grads(params, step)
        norms.append(check_step(f"boundary set, step {step}, lr {opt.param_groups[0]['lr']:.2e}", opt).item())
        sched.step()
    assert any(n > MAX_NORM for n in norms) and any(n + 1e-6 <= MAX_NORM for n in norms), norms        # coef < 1 and coef == 1
    assert opt.state[params[16]]["step"].item() == 3 and opt.state[params[0]]["step"].item() == 5
    assert params[13] not in opt.state and params[14] not in opt.state
    assert (params[12] == 0).all() and (opt.state[params[12]]["exp_avg_sq"] == 0).all()
    # a step without a clip since the last one runs with coef = 1
    set_boundary_grads(params, 4)
    check_step("boundary set, step without a clip", opt, clip=False)


def test_real_parameter_set():
    from relation_detr_amd import build_relation_transformer
    net = build_relation_transformer().to(DEV)
    params = list(net.parameters())
    assert len(params) == 317 and sum(p.numel() for p in params) == 19_752_960 and sum(p.numel() == 91 for p in params) == 8
    opt = FusedAdamW(relation_param_groups(net, 1e-4), lr=1e-4, weight_decay=1e-4, fused=True)
    assert sum(len(g["params"]) for g in opt.param_groups) == 317
    g = torch.Generator(device=DEV).manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=DEV) * 1e-3
    norm = check_step("R50 parameter set, first step", opt)
    assert norm.item() > MAX_NORM


def test_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        params, opt, sched = boundary_run()
        seen = []
        for step in range(2):
            set_boundary_grads(params, step)
            norm = opt.clip_grad_norm_(MAX_NORM)
            seen += [norm.clone(), opt.clip_coef.clone()]
            opt.step()
            sched.step()
        for p in params:
            s = opt.state.get(p) or {}
            seen += [p.detach().clone()] + ([s["exp_avg"].clone(), s["exp_avg_sq"].clone()] if s else [])
        runs.append(seen)
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


def test_state_dict_moves_between_the_routes_and_torch():
    """Two fused steps, then the state dict goes to a second fused optimizer, which continues with the same bits and within the
    bounds, and loads into torch.optim.AdamW."""
    params, opt, sched = boundary_run()
    for step in range(2):
        set_boundary_grads(params, step)
        opt.clip_grad_norm_(MAX_NORM)
        opt.step()
    saved = copy.deepcopy(opt.state_dict())
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and s["step"].device.type == "cpu" and s["step"].dtype == F32
               for s in saved["state"].values())
    twin_params, twin_groups = boundary_params()
    with torch.no_grad():
        for q, p in zip(twin_params, params):
            q.copy_(p)
    twin = FusedAdamW(twin_groups, lr=1e-3, weight_decay=1e-2, fused=True)
    twin.load_state_dict(saved)
    plain = torch.optim.AdamW(boundary_params()[1], lr=1e-3, weight_decay=1e-2)
    plain.load_state_dict(copy.deepcopy(saved))
    assert [g["lr"] for g in plain.param_groups] == [g["lr"] for g in opt.param_groups]
    assert plain.state_dict()["state"].keys() == saved["state"].keys()
    set_boundary_grads(params, 2)
    set_boundary_grads(twin_params, 2)
    na, nb = opt.clip_grad_norm_(MAX_NORM), twin.clip_grad_norm_(MAX_NORM)
    opt.step()
    twin.step()
    assert torch.equal(na, nb)
    for p, q in zip(params, twin_params):
        assert torch.equal(p, q)
        sa, sb = opt.state.get(p) or {}, twin.state.get(q) or {}
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    check_step("boundary set, step after a state-dict round trip", twin)


def test_step_invalidates_the_weight_caches():
    from test_denoising_host import head_inputs, tiny_head
    head = tiny_head(DEV, True)
    (feats, masks, pos), targets = head_inputs(DEV)
    opt = FusedAdamW(relation_param_groups(head, 1e-3), lr=1e-3, weight_decay=1e-4, fused=True)

    def eval_forward(h):
        h.eval()
        with torch.no_grad():
            logits, boxes = h(feats, masks, pos)
        return logits.clone(), boxes.clone()
    before = eval_forward(head)                                                 # fills the packed and merged weight caches
    head.train()
    train_step(head, opt, feats, masks, pos, targets)
    after = eval_forward(head)
    fresh = tiny_head(DEV, True)
    fresh.load_state_dict(head.state_dict())
    want = eval_forward(fresh)
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])


def test_routes_agree_on_the_tiny_head():
    from test_denoising_host import EXPECTED_KEYS, head_inputs, tiny_head
    head = tiny_head(DEV, True).train()
    (feats, masks, pos), targets = head_inputs(DEV)
    losses = head(feats, masks, pos, targets)
    sum(losses.values()).backward()
    twin = copy.deepcopy(head)
    for p, q in zip(head.parameters(), twin.parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    make = lambda h, fused: FusedAdamW(relation_param_groups(h, 1e-4), lr=1e-4, weight_decay=1e-4, fused=fused)
    a, b = make(head, True), make(twin, False)
    assert a._on_fused_route() and not b._on_fused_route()
    rows = snapshot(a)
    na, nb = a.clip_grad_norm_(MAX_NORM), b.clip_grad_norm_(MAX_NORM)
    a.step()
    b.step()
    n64, want = torch_route_step(a, rows, MAX_NORM, F64)
    worst = Worst()
    worst.add("norm", na, n64, nb, n64.abs())
    i = 0
    for group, other in zip(a.param_groups, b.param_groups):
        for p, q in zip(group["params"], other["params"]):
            if rows[i]["g"] is not None:
                p64, m64, v64, g64 = want[i]
                step_size, bias2_sqrt = step_scalars(group["lr"], *group["betas"], group["eps"], group["weight_decay"], 1.0)[4:6]
                scale = rows[i]["p"].to(F64).abs() + step_size * g64.abs() / (v64.sqrt() / bias2_sqrt + group["eps"])
                bound = torch.maximum(4 * (q.detach().to(F64) - p64).abs(), FLOOR * scale)
                frac = torch.where(p.detach() == q.detach(), torch.zeros_like(bound), (p.detach().to(F64) - q.detach().to(F64)).abs() / bound)
                worst.worst["param against the torch route"] = torch.maximum(worst.worst.get("param against the torch route", frac.new_zeros(1)),
                                                                             frac.max().reshape(1))
                worst.add("param", p.detach(), p64, q.detach(), scale)
            else:
                assert torch.equal(p, q)
            i += 1
    bound = torch.maximum(4 * (nb.to(F64) - n64).abs(), FLOOR * n64.abs())
    worst.worst["norm against the torch route"] = ((na.to(F64) - nb.to(F64)).abs() / bound).reshape(1)
    worst.report("tiny head, fused route against the torch route")

    losses, norm = train_step(head, a, feats, masks, pos, targets)
    assert set(losses) == EXPECTED_KEYS and norm.ndim == 0 and torch.isfinite(norm) and all(torch.isfinite(v) for v in losses.values())
