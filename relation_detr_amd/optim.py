"""The optimizer step of the reference's training loop: global-norm clip and AdamW (csrc/optim.hip).

The reference's loop goes on behind the loss (``util/engine.py:57-61``, ``configs/train_config.py:14,42-46``): ``zero_grad``,
``backward``, ``clip_grad_norm_(model.parameters(), 0.1)`` and ``AdamW(lr=1e-4, weight_decay=1e-4).step()`` over the six parameter
groups of ``optimizer/param_dict.py:81-148``.  ``FusedAdamW`` is that optimizer, ``relation_param_groups`` those groups and
``train_step`` one pass of the loop over a ``RelationDETRHead``.

Two routes, chosen by the constructor's ``fused`` (CPU parameters always take the second):

* fused -- one table in device memory lists every parameter tensor once (addresses of parameter and moments, numel, alignment) and,
  rewritten every step, its gradient's address and its group's scalars; a chunk map sends chunk ``c`` to (tensor, first element).
  ``clip_grad_norm_`` launches the per-chunk sum of squares and the one-workgroup coefficient kernel, ``step`` the update, which reads
  the coefficient on the device: three launches and one asynchronous copy from pinned memory per step, whatever the tensor count,
  and no host synchronisation.  The ``step`` counts of the states are 0-dim views of one host buffer, read and advanced in one
  operation each.  The kernels write parameters through raw pointers, so ``step`` bumps the version counter of every
  tensor it wrote: the packed and merged weight caches of this package key on ``_version``.
* torch -- ``torch.nn.utils.clip_grad_norm_`` and torch's functional AdamW, on any device and dtype.  It is what the fused route is
  timed and, in float64, checked against.

One deviation on the fused route: ``p.grad`` keeps the unclipped gradient (the clip coefficient is applied in registers), where torch
scales the gradients in place.  Non-finite gradients behave as in torch: a NaN norm gives a NaN coefficient and NaN parameters.  Not
built: ``amsgrad``, ``maximize``, bf16 parameters or master weights, HIP-graph capture of the step, gradient accumulation helpers.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib

CHUNK = 8192                     # elements of one chunk: one workgroup's unit of work, a multiple of 4 (16-byte vectors)
GRID_CAP = 0                     # workgroups per launch; 0: the library's default (2048)

# the three tables of include/relation_detr_amd.h: rdetr_optim_tensor, rdetr_optim_step, rdetr_optim_chunk
TENSOR_DT = np.dtype([("param", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"), ("aligned16", "<i4"), ("reserved", "<i4")])
STEP_DT = np.dtype([("grad", "<u8"), ("decay", "<f4"), ("one_minus_beta1", "<f4"), ("beta2", "<f4"), ("one_minus_beta2", "<f4"),
                    ("step_size", "<f4"), ("bias2_sqrt", "<f4"), ("eps", "<f4"), ("reserved", "<f4")])
CHUNK_DT = np.dtype([("first", "<i8"), ("tensor", "<i4"), ("reserved", "<i4")])
_SCALARS = ("decay", "one_minus_beta1", "beta2", "one_minus_beta2", "step_size", "bias2_sqrt", "eps")
_REFUSED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable")


def build_chunk_map(numels: Sequence[int], chunk: int = CHUNK) -> np.ndarray:
    """The chunk map of tensors with ``numels`` elements: chunk ``c`` covers ``[first, min(first + chunk, numel))`` of ``tensor``.
    Tensors appear in order, every element in exactly one chunk, no chunk crosses a tensor, a tensor without elements has none."""
    if chunk <= 0 or chunk % 4:
        raise ValueError(f"chunk has to be a positive multiple of 4, got {chunk}")
    numels = np.asarray(list(numels), dtype=np.int64)
    if (numels < 0).any():
        raise ValueError("negative numel")
    counts = (numels + chunk - 1) // chunk
    out = np.zeros(int(counts.sum()), dtype=CHUNK_DT)
    out["tensor"] = np.repeat(np.arange(len(numels), dtype=np.int32), counts)
    starts = np.cumsum(counts) - counts                                         # index of each tensor's first chunk
    out["first"] = (np.arange(len(out), dtype=np.int64) - np.repeat(starts, counts)) * chunk
    return out


def step_scalars(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, t: float) -> Tuple[float, ...]:
    """The scalars of step ``t`` as torch's single-tensor AdamW forms them in Python doubles, in the order of ``rdetr_optim_step``."""
    return (1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5, eps)


def fused_refusal(p: Tensor) -> Optional[str]:
    """Why the fused route cannot take parameter ``p``, or None: it wants fp32, dense and contiguous on a GPU."""
    if p.dtype != torch.float32:
        return f"dtype {p.dtype}, the kernels are fp32"
    if p.layout != torch.strided:
        return f"layout {p.layout}, the kernels want dense tensors"
    if not p.is_contiguous():
        return "not contiguous"
    if not p.is_cuda:
        return f"on {p.device}, not on a GPU"
    return None


def relation_param_groups(model: torch.nn.Module, lr: float) -> List[Dict]:
    """The six parameter groups of the reference (``optimizer/param_dict.py:81-148``) by parameter name, in its order: the rest;
    backbone; backbone norms and biases; ``reference_points`` / ``sampling_offsets`` projections; their biases; the other norms and
    biases.  Backbone and projection groups train at ``0.1 * lr``, norm and bias groups without weight decay; the keys a group
    leaves out come from the optimizer's defaults.  Frozen parameters are left out, empty groups dropped.  As in the reference, a
    ``reference_points`` / ``sampling_offsets`` parameter inside the backbone lands in no group."""
    buckets: List[List[Tensor]] = [[] for _ in range(6)]
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        backbone = "backbone" in name
        projection = "reference_points" in name or "sampling_offsets" in name
        no_decay = "norm" in name or "bias" in name
        if backbone and projection:
            continue
        if backbone:
            buckets[2 if no_decay else 1].append(p)
        elif projection:
            buckets[4 if no_decay else 3].append(p)
        else:
            buckets[5 if no_decay else 0].append(p)
    extra = [{}, {"lr": lr * 0.1}, {"lr": lr * 0.1, "weight_decay": 0}, {"lr": lr * 0.1}, {"lr": lr * 0.1, "weight_decay": 0}, {"weight_decay": 0}]
    return [{"params": params, **kw} for params, kw in zip(buckets, extra) if params]


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` with the global-norm clip attached: ``clip_grad_norm_(max_norm)`` then ``step()``.

    ``param_groups`` and ``state`` (``step``, ``exp_avg``, ``exp_avg_sq``) have ``torch.optim.AdamW``'s layout, so ``state_dict()``
    moves between the two both ways and torch's LR schedulers drive it.  ``fused``: see the module docstring."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, *, maximize: bool = False, capturable: bool = False, differentiable: bool = False,
                 fused: bool = True):
        if isinstance(lr, Tensor):
            raise ValueError("FusedAdamW: a tensor lr is not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.fused = bool(fused)
        self._armed = None                   # the workspace whose last two floats are {total_norm, coef} for the next step()
        self._prepared = None                # what clip_grad_norm_ put on the device, for the step() behind it
        self._tables = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=capturable, differentiable=differentiable, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._check_groups()

    # ------------------------------------------------------------------------------------------------------------------ checks
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        self._tables = self._prepared = None
        if hasattr(self, "fused"):
            self._check_groups()

    def _params(self) -> List[Tensor]:
        return [p for group in self.param_groups for p in group["params"]]

    def _on_fused_route(self) -> bool:
        """Decided by the first parameter; ``_check_groups`` has seen to it that the others are on the same side."""
        first = self._first_param()
        return self.fused and first is not None and first.device.type != "cpu"

    def _first_param(self) -> Optional[Tensor]:
        return next((p for group in self.param_groups for p in group["params"]), None)

    def _check_flags(self) -> None:
        for group in self.param_groups:
            for flag in _REFUSED_FLAGS:
                if group.get(flag):
                    raise ValueError(f"FusedAdamW: {flag} is not supported")
            if isinstance(group["lr"], Tensor):
                raise ValueError("FusedAdamW: a tensor lr is not supported")

    def _check_groups(self) -> None:
        self._check_flags()
        params = self._params()
        if self.fused and any(p.device.type != "cpu" for p in params):
            for p in params:
                why = fused_refusal(p)
                if why is not None:
                    raise ValueError(f"FusedAdamW(fused=True): parameter of shape {tuple(p.shape)} is {why}")
            if len({p.device for p in params}) != 1:
                raise ValueError("FusedAdamW(fused=True): the parameters have to be on one GPU")

    @staticmethod
    def _grad_of(p: Tensor) -> Optional[Tensor]:
        g = p.grad
        if g is not None and (g.is_sparse or g.layout != torch.strided):
            raise ValueError("FusedAdamW does not support sparse gradients")
        return g

    def _init_state(self, p: Tensor) -> Dict:
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    # ------------------------------------------------------------------------------------------------------------------ torch route
    def _clip_torch(self, max_norm: float) -> Tensor:
        params = self._params()
        for p in params:
            self._grad_of(p)
        return torch.nn.utils.clip_grad_norm_(params, max_norm)

    def _step_torch(self) -> None:
        from torch.optim.adamw import adamw
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, steps = [], [], [], [], []
            for p in group["params"]:
                g = self._grad_of(p)
                if g is None:
                    continue
                state = self._init_state(p)
                params.append(p)
                grads.append(g)
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                steps.append(state["step"])
            if not params:
                continue
            beta1, beta2 = group["betas"]
            adamw(params, grads, exp_avgs, exp_avg_sqs, [], steps, foreach=None, capturable=False, differentiable=False, fused=None,
                  has_complex=any(torch.is_complex(p) for p in params), amsgrad=False, beta1=beta1, beta2=beta2, lr=group["lr"],
                  weight_decay=group["weight_decay"], eps=group["eps"], maximize=False)

    # ------------------------------------------------------------------------------------------------------------------ fused route
    def _gather(self):
        """Parameters, their gradients as the kernels read them (contiguous fp32 on the parameters' device, or None), the states, and
        what ``_prepared_still_holds`` compares: the ``p.grad`` objects and the contiguous copies made for them."""
        params = self._params()
        device = params[0].device
        seen = [p.grad for p in params]
        grads, states, copies = [], [], {}
        known = self._tables["states"] if self._tables is not None and len(self._tables["states"]) == len(params) else [None] * len(params)
        for i, (p, g) in enumerate(zip(params, seen)):
            if g is None:
                grads.append(None)
                states.append(known[i] or self.state.get(p) or None)
                continue
            if g.layout != torch.strided:
                raise ValueError("FusedAdamW does not support sparse gradients")
            if g.dtype != torch.float32 or g.device != device:
                raise ValueError(f"FusedAdamW(fused=True): gradient of dtype {g.dtype} on {g.device}, expected fp32 on {device}")
            if not g.is_contiguous():                                           # made contiguous for the step
                copies[i] = (g._version, g.contiguous())
                g = copies[i][1]
            grads.append(g)
            states.append(known[i] or self._init_state(p))
        return params, seen, grads, states, copies

    def _group_keys(self) -> List[Tuple[float, ...]]:
        return [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])) for g in self.param_groups]

    def _build_tables(self, params, states, signature):
        device = params[0].device
        chunk_map = build_chunk_map([p.numel() for p in params], CHUNK)
        tensors = np.zeros(len(params), dtype=TENSOR_DT)
        sig = np.asarray(signature, dtype=np.uint64).reshape(len(params), 3)
        tensors["param"], tensors["exp_avg"], tensors["exp_avg_sq"] = sig[:, 0], sig[:, 1], sig[:, 2]
        tensors["numel"] = [p.numel() for p in params]
        tensors["aligned16"] = ((sig % 16) == 0).all(axis=1)
        static = np.concatenate((chunk_map.view(np.uint8), tensors.view(np.uint8)))
        step_bytes = len(params) * STEP_DT.itemsize
        if self._tables is None or self._tables["table"].numel() != len(static) + step_bytes or self._tables["table"].device != device:
            table = torch.empty(len(static) + step_bytes, dtype=torch.uint8, device=device)
            pinned = [torch.empty(step_bytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
            events, turn = [None, None], 0
        else:
            t = self._tables
            table, pinned, events, turn = t["table"], t["pinned"], t["events"], t["turn"]
        table[:len(static)].copy_(torch.from_numpy(static))
        # the step counts move into one host buffer, each state's `step` a 0-dim view of it: one read and one add per step for all
        have = [i for i, s in enumerate(states) if s]
        steps = torch.zeros(len(params), dtype=torch.float32)
        if have:
            steps[have] = torch.tensor([float(states[i]["step"]) for i in have], dtype=torch.float32)
        for i in have:
            states[i]["step"] = steps[i]
        base = table.data_ptr()
        group_of = np.repeat(np.arange(len(self.param_groups)), [len(g["params"]) for g in self.param_groups])
        self._tables = dict(signature=signature, table=table, pinned=pinned, pinned_np=[x.numpy() for x in pinned], events=events, turn=turn,
                            group_of=group_of, states=list(states), steps=steps.numpy(),
                            n_tensors=len(params), n_chunks=len(chunk_map), map_ptr=base, tensors_ptr=base + chunk_map.nbytes,
                            steps_ptr=base + len(static), steps_off=len(static), scalars={})

    def _prepare(self) -> Dict:
        """Bring the device tables up to date for the step about to run: the static part when a tensor moved or a state appeared, the
        per-step part in one asynchronous copy from pinned memory.  ``clip_grad_norm_`` leaves what it prepared for ``step``."""
        params, seen, grads, states, copies = self._gather()
        signature = []
        for p, s in zip(params, states):
            signature += [p.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()] if s else [p.data_ptr(), 0, 0]
        if self._tables is None or self._tables["signature"] != signature:
            for p, s in zip(params, states):
                if s:
                    for m in (s["exp_avg"], s["exp_avg_sq"]):
                        if m.dtype != torch.float32 or m.device != p.device or not m.is_contiguous() or m.numel() != p.numel():
                            raise ValueError("FusedAdamW(fused=True): optimizer state has to be contiguous fp32 on the parameter's GPU")
            self._build_tables(params, states, signature)
        t = self._tables
        live = [i for i, g in enumerate(grads) if g is not None]
        host = np.zeros(len(params), dtype=STEP_DT)
        keys = self._group_keys()
        if live:
            now = t["steps"][live].astype(np.float64) + 1.0
            group_of = t["group_of"][live]
            rows = np.zeros((len(live), len(_SCALARS)), dtype=np.float32)
            for gi, key0 in enumerate(keys):
                mine = group_of == gi
                for step_no in np.unique(now[mine]):
                    key = key0 + (float(step_no),)
                    scalars = t["scalars"].get(key)
                    if scalars is None:
                        if len(t["scalars"]) > 64:
                            t["scalars"].clear()
                        scalars = t["scalars"][key] = np.asarray(step_scalars(*key), dtype=np.float64).astype(np.float32)
                    rows[mine & (now == step_no)] = scalars
            ptrs = np.zeros(len(params), dtype=np.uint64)
            ptrs[live] = [grads[i].data_ptr() for i in live]
            host["grad"] = ptrs
            for k, name in enumerate(_SCALARS):
                host[name][live] = rows[:, k]
        turn = t["turn"]
        if t["events"][turn] is not None:
            t["events"][turn].synchronize()                                       # the copy that last read this pinned buffer is done
        t["pinned_np"][turn][:] = host.view(np.uint8)
        t["table"][t["steps_off"]:].copy_(t["pinned"][turn], non_blocking=True)
        if t["events"][turn] is None:
            t["events"][turn] = torch.cuda.Event()
        t["events"][turn].record(torch.cuda.current_stream(params[0].device))
        t["turn"] = 1 - turn
        return dict(params=params, seen=seen, grads=grads, states=states, copies=copies, live=live, keys=keys)

    def _prepared_still_holds(self, ctx: Optional[Dict]) -> bool:
        """Whether what ``clip_grad_norm_`` put on the device still describes the step: the same gradient objects, group settings and
        contiguous copies.  A gradient rewritten in place keeps its address and is read as it is now."""
        if ctx is None or self._tables is None or ctx["keys"] != self._group_keys():
            return False
        params = self._params()
        if len(params) != len(ctx["params"]) or any(p is not q or p.grad is not g for p, q, g in zip(params, ctx["params"], ctx["seen"])):
            return False
        return all(ctx["seen"][i]._version == version for i, (version, _) in ctx["copies"].items())

    def _clip_fused(self, max_norm: float) -> Tensor:
        device = self._first_param().device
        lib = _lib.load()
        with torch.cuda.device(device):
            self._prepared = None
            ctx = self._prepare()
            t = self._tables
            stream = torch.cuda.current_stream(device).cuda_stream
            n_chunks = t["n_chunks"]
            ws_bytes = max(int(lib.rdetr_optim_workspace_bytes(n_chunks)), 8)
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=device)
            _lib.check(lib.rdetr_grad_sqnorm_f32(t["tensors_ptr"], t["steps_ptr"], t["map_ptr"], t["n_tensors"], n_chunks, CHUNK, GRID_CAP,
                                                 ws.data_ptr(), ws_bytes, stream), "rdetr_grad_sqnorm_f32")
            _lib.check(lib.rdetr_grad_clip_coef(ws.data_ptr(), ws_bytes, n_chunks, float(max_norm), stream), "rdetr_grad_clip_coef")
        self._armed, self._prepared = ws, ctx
        return ws[n_chunks]

    def _step_fused(self) -> None:
        device = self._first_param().device
        lib = _lib.load()
        armed, ctx = self._armed, getattr(self, "_prepared", None)
        self._armed = self._prepared = None
        with torch.cuda.device(device):
            if not self._prepared_still_holds(ctx):
                ctx = self._prepare()
            t = self._tables
            stream = torch.cuda.current_stream(device).cuda_stream
            coef = ctypes.c_void_p(armed.data_ptr() + 4 * t["n_chunks"]) if armed is not None else None
            _lib.check(lib.rdetr_adamw_step_f32(t["tensors_ptr"], t["steps_ptr"], t["map_ptr"], t["n_tensors"], t["n_chunks"], CHUNK,
                                                GRID_CAP, coef, stream), "rdetr_adamw_step_f32")
        params, states, live = ctx["params"], ctx["states"], ctx["live"]
        if live:
            t["steps"][live] += 1.0                                              # every live state's `step`, through the shared buffer
            written = [x for i in live for x in (params[i], states[i]["exp_avg"], states[i]["exp_avg_sq"])]
            torch.autograd.graph.increment_version(written)                      # the weight caches key on _version

    # ------------------------------------------------------------------------------------------------------------------ interface
    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float) -> Tensor:
        """The total 2-norm of the gradients of this optimizer's parameters, taken in group order, as a 0-dim tensor on their device,
        no synchronisation.  Torch route:
        ``torch.nn.utils.clip_grad_norm_``, the gradients scaled in place.  Fused route: the gradients stay as they are and the
        coefficient ``min(1, max_norm / (norm + 1e-6))`` is armed for the next ``step()``; without a call since the last step it is 1."""
        if self._on_fused_route():
            return self._clip_fused(max_norm)
        return self._clip_torch(max_norm)

    @property
    def clip_coef(self) -> Optional[Tensor]:
        """Fused route: the coefficient armed for the next ``step()`` as a 0-dim device tensor, None when there is none."""
        return None if self._armed is None else self._armed[-1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_flags()
        if self._on_fused_route():
            self._step_fused()
        else:
            self._step_torch()
        return loss

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._tables = self._prepared = None
        self._check_groups()


def train_step(head, optimizer: FusedAdamW, feats, masks, pos, targets, max_norm: float = 0.1, noise=None):
    """One pass of the reference's loop (``util/engine.py:46-61``) over a ``RelationDETRHead`` in training mode: ``zero_grad``, the
    head's forward, the sum of the loss dict, ``backward``, the clip when ``max_norm > 0``, ``step``.  Returns ``(loss_dict,
    total_norm)``, ``total_norm`` a 0-dim tensor or None without a clip; nothing here waits for the device.  With ``pos=None``
    the module builds its own pyramid: ``head`` is a ``RelationDETR``, ``feats`` the backbone's feature maps and ``masks`` the image-level
    padding mask."""
    optimizer.zero_grad()
    loss_dict = head(feats, masks, targets, noise=noise) if pos is None else head(feats, masks, pos, targets, noise=noise)
    sum(loss_dict.values()).backward()
    total_norm = optimizer.clip_grad_norm_(max_norm) if max_norm > 0 else None
    optimizer.step()
    return loss_dict, total_norm
