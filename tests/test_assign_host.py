"""CPU checks of the device matcher's host side (relation_detr_amd/criterion.py ``assign_match``, csrc/assign.hip's C entry): the
symbol declared once, bound and exported with the ABI version and the Options fields unchanged, the argument refusals of the C
entry, the scipy route of ``assign_match`` against the reference's recorded assignments (tests/golden/g10_criterion.npz), and the
``matcher`` keyword of ``RelationCriterion``.  The kernel itself is checked in tests/test_gpu_assign.py."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import relation_detr_amd
from conftest import load_golden
from relation_detr_amd import _lib, criterion as crit, options
from relation_detr_amd.criterion import RelationCriterion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [f"dec{l}" for l in range(3)] + ["enc"] + [f"hyb{l}" for l in range(3)] + ["hyb_enc"]
COUNTS = [3, 2]


@pytest.fixture(scope="module")
def g10():
    return load_golden("g10_criterion.npz")


def fixture_stack(z, name):
    """cost32.<name>.<b> of the two images stacked [2, N, 3] (image 1's third column is padding), and the recorded tables [2, N]."""
    N = z[f"cost32.{name}.0"].shape[0]
    cost = torch.zeros(2, N, 3, dtype=torch.float32)
    for b, g in enumerate(COUNTS):
        cost[b, :, :g] = torch.from_numpy(z[f"cost32.{name}.{b}"])
    want = np.stack([z[f"match.{name}.{b}"] for b in range(2)])
    return cost, want


def test_symbol_is_declared_once_bound_and_exported():
    name = "rdetr_assign_match"
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert len(re.findall(r"^int " + name + r"\s*\(", header, re.M)) == 1
    assert name in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert callable(getattr(_lib.load(), name))


def test_abi_options_exports_and_shadow_tables():
    header = open(os.path.join(ROOT, "include", "relation_detr_amd.h")).read()
    assert "#define RDETR_ABI_VERSION 3" in header and _lib.load().rdetr_abi_version() == 3
    assert len(dataclasses.fields(options.Options)) == 25                   # the matcher is a constructor argument
    assert "assign_match" in relation_detr_amd.__all__ and relation_detr_amd.assign_match is crit.assign_match
    assert "hungarian_match" in relation_detr_amd.__all__
    import test_shadow_complete as t
    t.test_every_ops_function_is_classified()
    t.test_every_rdetr_symbol_is_under_the_tripwire_or_excluded()
    t.test_every_training_module_function_is_classified()


def test_argument_refusals():
    fn = _lib.load().rdetr_assign_match
    one = ctypes.c_void_p(16)

    def call(cost=one, count=one, R=4, B=2, N=8, G=3, repeat=1, skip=0, dn=(0, 0), match=one, ld=None, status=one):
        return fn(cost, count, R, B, N, G, repeat, skip, dn[0], dn[1], match, skip + N if ld is None else ld, status, None)
    assert call(R=0) == 0 and call(R=0, cost=None, match=None, status=None) == 0          # nothing to do, nothing launched
    assert call(cost=None) == -1 and call(match=None) == -1 and call(status=None) == -1 and call(count=None) == -1
    assert call(B=0) == -1 and call(R=3) == -1 and call(repeat=0) == -1 and call(G=0) == -1 and call(N=-1) == -1
    assert call(ld=7) == -1 and call(skip=6, dn=(2, 3), ld=13) == -1
    assert call(skip=6, dn=(2, 2)) == -1 and call(skip=6) == -1 and call(skip=0, dn=(2, 3)) == -1
    assert call(N=crit.MAX_ASSIGN + 1) == -2                                               # the named limits, either side
    assert call(G=342, repeat=6) == -2 and call(G=crit.MAX_ASSIGN + 1) == -2
    assert call(cost=ctypes.c_void_p(18)) == -2 and call(match=ctypes.c_void_p(6)) == -2 and call(status=ctypes.c_void_p(2)) == -2
    assert crit.MAX_ASSIGN == 2048


@pytest.mark.parametrize("name", SETS)
def test_cpu_route_reproduces_the_recorded_assignments(g10, name):
    cost, want = fixture_stack(g10, name)
    repeat = 6 if name.startswith("hyb") else 1
    match, status = crit.assign_match(cost, COUNTS, repeat=repeat)
    assert match.dtype == torch.int32 and status.dtype == torch.int32 and tuple(match.shape) == want.shape
    assert np.array_equal(match.numpy(), want) and status.tolist() == [0, 0]              # margins >= 1e-3: the maps compare exactly
    again, _ = crit.assign_match(cost, torch.tensor(COUNTS, dtype=torch.int32), repeat=repeat, fused=False)
    assert torch.equal(again, match)
    for b in range(2):
        assert float(g10[f"margin.{name}.{b}"]) >= 1e-3


def test_cpu_route_denoising_fill_and_out_slice(g10):
    """dn_meta = (2, 3), counts [3, 2]: what _forward_fused built on the host before this function had it."""
    cost, want = fixture_stack(g10, "dec0")
    cost6 = cost.repeat(3, 1, 1)                                                          # R = 6: rows 0, 2, 4 are image 0
    N = cost.shape[1]
    wide = torch.full((6, 6 + N + 4), 7, dtype=torch.int32)
    match, status = crit.assign_match(cost6, COUNTS, skip=6, dn_meta=(2, 3), out=wide[:, 1:])
    assert match.data_ptr() == wide[:, 1:].data_ptr() and tuple(match.shape) == (6, 6 + N) and status.tolist() == [0] * 6
    slot = torch.arange(3, dtype=torch.int32)
    for r in range(6):
        fixed = torch.where(slot < COUNTS[r % 2], slot, slot.new_tensor(-1)).repeat(2)
        assert torch.equal(match[r, :6], fixed)
        assert np.array_equal(match[r, 6:].numpy(), want[r % 2])
    assert match[1, :6].tolist() == [0, 1, -1, 0, 1, -1]
    assert (wide[:, 0] == 7).all() and (wide[:, 1 + 6 + N:] == 7).all()                    # nothing outside skip + N columns
    with pytest.raises(ValueError):
        crit.assign_match(cost6, COUNTS, skip=6, dn_meta=(2, 2))
    with pytest.raises(ValueError):
        crit.assign_match(cost6, COUNTS, skip=6)
    with pytest.raises(ValueError):
        crit.assign_match(cost6, COUNTS, repeat=0)


def test_cpu_route_empty_image_more_copies_than_queries_and_status():
    g = torch.Generator().manual_seed(3)
    cost = torch.rand(3, 8, 3, generator=g)
    match, status = crit.assign_match(cost, [3, 0, 2], repeat=6)                          # 18 and 12 copies for 8 queries
    assert (match[1] == -1).all() and (match[0] >= 0).all() and (match[2] >= 0).all() and (match[2] < 2).all()
    assert status.tolist() == [0, 0, 0]
    cost[2, 4, 1] = float("nan")
    match2, status2 = crit.assign_match(cost, [3, 0, 2], repeat=6)
    assert status2.tolist() == [0, 0, 1] and (match2[2] == -1).all() and torch.equal(match2[:2], match[:2])


def test_matcher_keyword():
    with pytest.raises(ValueError):
        RelationCriterion(5, matcher="x")
    assert RelationCriterion(5).matcher == "scipy" and RelationCriterion(5, matcher="device").matcher == "device"
    import test_criterion_host as host
    losses = {}
    for matcher in ("scipy", "device"):
        outs, g = host.random_outputs(n_dn=6, dtype=torch.float32)
        targets = host.random_targets((3, 2), 5, g, dtype=torch.float32)
        values = RelationCriterion(5, matcher=matcher, fused=False)(tuple(outs), targets, (2, 3))
        torch.stack(list(values.values())).sum().backward()
        losses[matcher] = (values, [t.grad for t in outs])
    assert set(losses["device"][0]) == set(losses["scipy"][0]) and len(losses["scipy"][0]) == 24
    for k, v in losses["scipy"][0].items():
        assert torch.equal(losses["device"][0][k], v), k                                  # CPU tensors: one route, the same bits
    for a, b in zip(losses["device"][1], losses["scipy"][1]):
        assert torch.equal(a, b)
