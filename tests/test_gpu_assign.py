"""GPU checks of the device matcher (csrc/assign.hip, ``criterion.assign_match``, ``RelationCriterion(matcher="device")``).

The checker is scipy's ``linear_sum_assignment`` on the same fp32 costs copied to the host (``assign_match(..., fused=False)``).
The kernel runs scipy's method in scipy's arithmetic (fp64 over the fp32 costs), so nothing here has a tolerance but the total
cost, whose two sums add the same at most 2048 fp32 values in fp64 in another order: 1e-9 of the sum of their magnitudes, far
below any gap between two assignments of costs that differ in the third decimal."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETS = [f"dec{l}" for l in range(3)] + ["enc"] + [f"hyb{l}" for l in range(3)] + ["hyb_enc"]
# (N, gt counts of the B images, repeat, R, Gmax - max(counts))
RANDOM_CASES = [
    (37, [3, 0], 1, 2, 0),
    (8, [3], 6, 1, 0),                  # 18 copies for 8 queries: the queries are the short side
    (130, [1, 17], 6, 2, 0),            # 102 copies < 130 queries
    (70, [17, 5], 6, 2, 0),             # 102 > 70 and 30 < 70 in one launch: both orientations
    (5, [5], 1, 1, 0),                  # square
    (1, [1], 1, 1, 0),
    (257, [20, 7], 6, 2, 0),            # one past a 256-lane stride
    (300, [20, 20], 1, 6, 0),           # R = 6: row r is image r % 2
    (45, [4, 9], 2, 4, 3),              # Gmax larger than every count: the padded columns hold NaN and are never read
]


def crit():
    from relation_detr_amd import criterion
    return criterion


def solve_both(cost, counts, repeat, **kw):
    """(device table, device status, scipy's table) of a device cost stack."""
    c = crit()
    gt_count = torch.tensor(counts, dtype=torch.int32, device=DEV)
    match, status = c.assign_match(cost, gt_count, repeat=repeat, **kw)
    used = cost.cpu().clone()
    for r in range(cost.shape[0]):
        used[r, :, counts[r % len(counts)]:] = 0                                       # scipy never sees the padding either
    want, _ = c.assign_match(used, counts, repeat=repeat, fused=False, **{k: v for k, v in kw.items() if k != "out"})
    return match, status, want


def check_assignment(cost, counts, repeat, match, want):
    """(a) validity, (b) the total cost against scipy's, (c) the same pairs."""
    R, N, _ = cost.shape
    host, got, ref = cost.cpu().double().numpy(), match.cpu().numpy(), want.numpy()
    assert got.shape == ref.shape == (R, N) and got.dtype == np.int32
    for r in range(R):
        g = counts[r % len(counts)]
        m = got[r]
        assert ((m >= -1) & (m < max(g, 1))).all() and (g > 0 or (m == -1).all()), r
        per_target = np.bincount(m[m >= 0], minlength=max(g, 1))[:max(g, 1)]
        if g * repeat <= N:
            assert (per_target == (repeat if g else 0)).all(), (r, per_target)        # every target gets exactly `repeat` queries
        else:
            assert (m >= 0).all() and (per_target <= repeat).all(), (r, per_target)   # every query matched, no copy used twice
        q = np.nonzero(m >= 0)[0]
        q_ref = np.nonzero(ref[r] >= 0)[0]
        chosen, chosen_ref = host[r, q, m[q]], host[r, q_ref, ref[r][q_ref]]
        assert abs(chosen.sum() - chosen_ref.sum()) <= 1e-9 * np.abs(chosen_ref).sum(), (r, chosen.sum(), chosen_ref.sum())
        assert np.array_equal(m, ref[r]), r


def random_cost(R, N, Gmax, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(R, N, Gmax, generator=g) + 0.01 * torch.randn(R, N, Gmax, generator=g)


def test_fixture_assignments_from_the_recorded_costs():
    z = load_golden("g10_criterion.npz")
    counts = [3, 2]
    for name in SETS:
        N = z[f"cost32.{name}.0"].shape[0]
        cost = torch.zeros(2, N, 3)
        for b, g in enumerate(counts):
            cost[b, :, :g] = torch.from_numpy(z[f"cost32.{name}.{b}"])
        match, status = crit().assign_match(cost.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV),
                                            repeat=6 if name.startswith("hyb") else 1)
        assert match.dtype == torch.int32 and status.tolist() == [0, 0]
        for b in range(2):
            assert np.array_equal(match[b].cpu().numpy(), z[f"match.{name}.{b}"]), (name, b)


@pytest.mark.parametrize("N,counts,repeat,R,pad", RANDOM_CASES)
def test_random_continuous_costs(N, counts, repeat, R, pad):
    Gmax = max(1, max(counts)) + pad
    cost = random_cost(R, N, Gmax, seed=11 * N + repeat)
    if pad:
        for r in range(R):
            cost[r, :, counts[r % len(counts)]:] = float("nan")
    cost = cost.to(DEV)
    match, status, want = solve_both(cost, counts, repeat)
    assert status.tolist() == [0] * R
    check_assignment(cost, counts, repeat, match, want)


@pytest.mark.parametrize("repeat", [1, 3])
def test_contention_gives_long_augmenting_paths(repeat):
    """Every target wants the same few queries: cost[q, t] = base[q] + 1e-3 rand."""
    N, counts = 64, [20]
    g = torch.Generator().manual_seed(5 + repeat)
    cost = (torch.rand(1, N, 1, generator=g) + 1e-3 * torch.rand(1, N, 20, generator=g)).to(DEV)
    match, status, want = solve_both(cost, counts, repeat)
    assert status.tolist() == [0]
    check_assignment(cost, counts, repeat, match, want)


def test_ties_give_an_optimal_total_and_the_same_table_every_run():
    N, counts, repeat = 40, [12], 2
    g = torch.Generator().manual_seed(9)
    cost = torch.randint(0, 4, (1, N, 12), generator=g).float().to(DEV)
    match, status, want = solve_both(cost, counts, repeat)
    again, _ = crit().assign_match(cost, torch.tensor(counts, dtype=torch.int32, device=DEV), repeat=repeat)
    assert status.tolist() == [0] and torch.equal(match, again)
    m, ref, host = match[0].cpu().numpy(), want[0].numpy(), cost[0].cpu().double().numpy()
    assert (np.bincount(m[m >= 0], minlength=12) == repeat).all() and ((m >= -1) & (m < 12)).all()
    total = host[np.nonzero(m >= 0)[0], m[m >= 0]].sum()
    assert total == host[np.nonzero(ref >= 0)[0], ref[ref >= 0]].sum()                  # small integers: exact in any order


def test_denoising_fill_and_row_stride():
    N, counts, skip = 24, [3, 2], 6
    cost = random_cost(4, N, 3, seed=21).to(DEV)
    wide = torch.full((4, 1 + skip + N + 5), 7, dtype=torch.int32, device=DEV)
    match, status, want = solve_both(cost, counts, 1, skip=skip, dn_meta=(2, 3), out=wide[:, 1:])
    assert match.data_ptr() == wide[:, 1:].data_ptr() and tuple(match.shape) == (4, skip + N) and status.tolist() == [0] * 4
    assert match[:, :skip].tolist() == [[0, 1, 2, 0, 1, 2], [0, 1, -1, 0, 1, -1]] * 2
    assert torch.equal(match.cpu(), want)                                               # the host route builds the same table
    check_assignment(cost, counts, 1, match[:, skip:], want[:, skip:])
    assert (wide[:, 0] == 7).all() and (wide[:, 1 + skip + N:] == 7).all()               # nothing outside the row's skip + N entries


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_cost_that_is_not_finite_ends_its_row_alone(value):
    """The graceful path; that the kernel ends on any input is the loop bounds' doing, not this test's."""
    N, counts = 20, [4, 5, 3]
    cost = random_cost(3, N, 5, seed=31)
    good = cost.clone().to(DEV)
    cost[1, 13, 2] = value
    match, status = crit().assign_match(cost.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV))
    _, _, want = solve_both(good, counts, 1)
    assert status.tolist() == [0, 1, 0]
    assert (match[1] == -1).all()
    assert torch.equal(match[0].cpu(), want[0]) and torch.equal(match[2].cpu(), want[2])


@contextlib.contextmanager
def count_waits(monkeypatch):
    """Patches what waits for the device or copies from it to the host; yields the list of what was called."""
    seen = []

    def wrap(owner, name, is_wait):
        original = getattr(owner, name)

        def patched(*args, **kwargs):
            if is_wait(args, kwargs):
                seen.append(f"{getattr(owner, '__name__', owner)}.{name}")
            return original(*args, **kwargs)
        patch.setattr(owner, name, patched)

    def to_host(args, kwargs):
        target = [a for a in list(args[1:]) + list(kwargs.values()) if isinstance(a, (str, torch.device, torch.Tensor))]
        return args[0].is_cuda and any((torch.device(a) if isinstance(a, str) else getattr(a, "device", a)).type == "cpu" for a in target)
    always = lambda args, kwargs: True
    from_device = lambda args, kwargs: args[0].is_cuda
    with monkeypatch.context() as patch:
        wrap(torch.cuda.Event, "synchronize", always)
        wrap(torch.cuda.Stream, "synchronize", always)
        wrap(torch.cuda, "synchronize", always)
        for name in ("cpu", "item", "tolist", "numpy"):
            wrap(torch.Tensor, name, from_device)
        wrap(torch.Tensor, "to", to_host)
        wrap(torch.Tensor, "copy_", lambda args, kwargs: not args[0].is_cuda and torch.is_tensor(args[1]) and args[1].is_cuda)
        yield seen


@pytest.mark.parametrize("logit_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_criterion_with_the_device_matcher_is_the_default_bit_for_bit_and_never_waits(logit_dtype, monkeypatch):
    from relation_detr_amd import RelationCriterion
    z = load_golden("g10_criterion.npz")
    targets = [{"labels": torch.from_numpy(z[f"tgt.labels.{b}"]).to(DEV), "boxes": torch.from_numpy(z[f"tgt.boxes.{b}"]).to(DEV)}
               for b in range(2)]
    dn_meta = tuple(int(v) for v in z["dn_meta"])
    results, waits = {}, {}
    for matcher in ("scipy", "device"):
        outputs = [torch.from_numpy(z[f"out.{i}"]).to(DEV).to(logit_dtype if i % 2 == 0 else torch.float32).requires_grad_(True)
                   for i in range(8)]
        criterion = RelationCriterion(11, matcher=matcher)
        torch.cuda.synchronize()
        with count_waits(monkeypatch) as seen:
            losses = criterion(tuple(outputs), targets, dn_meta)
            torch.stack([v.float() for v in losses.values()]).sum().backward()
            waits[matcher] = list(seen)
        results[matcher] = (losses, [t.grad for t in outputs])
    assert "Event.synchronize" in waits["scipy"] and "Tensor.copy_" in waits["scipy"]      # the patches see the host route's wait and copy
    assert waits["device"] == []
    assert set(results["device"][0]) == set(results["scipy"][0]) and len(results["scipy"][0]) == 33
    for k, v in results["scipy"][0].items():
        assert torch.equal(results["device"][0][k], v), k
    for i, (a, b) in enumerate(zip(results["device"][1], results["scipy"][1])):
        assert a is not None and torch.equal(a, b), i


def test_shapes_beyond_the_kernel_take_the_host_route(monkeypatch):
    from relation_detr_amd import RelationCriterion, _lib
    c = crit()
    with pytest.raises(_lib.RdetrError):                                                   # the piece alone refuses ...
        c.assign_match(torch.zeros(1, c.MAX_ASSIGN + 1, 1, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV))
    lib, launches = _lib.load(), []
    entry = lib.rdetr_assign_match
    monkeypatch.setattr(lib, "rdetr_assign_match", lambda *a: launches.append(a[4]) or entry(*a))     # a[4]: N
    g = torch.Generator().manual_seed(2)
    targets = [{"labels": torch.randint(0, 3, (2,), generator=g).to(DEV),
                "boxes": torch.cat((torch.rand(2, 2, generator=g), 0.02 + 0.4 * torch.rand(2, 2, generator=g)), -1).to(DEV)}]
    for nq in (64, c.MAX_ASSIGN + 1):                                                      # ... and the criterion goes to scipy for that step
        logits = lambda *s: (2 * torch.randn(*s, 3, generator=g)).to(DEV)
        boxes = lambda *s: torch.cat((torch.rand(*s, 2, generator=g), 0.02 + 0.4 * torch.rand(*s, 2, generator=g)), -1).to(DEV)
        outs = (logits(1, 1, nq), boxes(1, 1, nq), logits(1, nq), boxes(1, nq), None, None, None, None)
        launches.clear()
        got = RelationCriterion(3, matcher="device")(outs, targets)
        want = RelationCriterion(3)(outs, targets)
        assert launches == ([64] if nq == 64 else []), launches                            # layers and proposals: one stack, one launch
        assert all(torch.equal(got[k], want[k]) for k in want) and set(got) == set(want)
