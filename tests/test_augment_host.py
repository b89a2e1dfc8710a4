"""Host side of the training augmentation (relation_detr_amd/frontend/augment.py): the size rule, the plans, the torch route and the
boxes against what the reference's own transform code recorded (tests/golden/g15_augment.npz, tools/gen_golden_augment.py), the
sampler's ranges, eval mode, and the unchanged parameters of ``batch_images``.  Needs no GPU and no built library.
tests/test_gpu_augment.py imports the fixture's references from here.

Pixels are held to the near-tie rule of tests/test_images_host.py on the LAST resize of a case.  A crop case resizes twice; its first
resize is recorded without any near tie inside the crop (``case_reference`` asserts that precondition first and fails as ill-posed
when it does not hold), so the intermediate uint8 crop is exact and is the source of the rule's float64 filter.
"""
import inspect

import numpy as np
import pytest
import torch

import relation_detr_amd
from conftest import load_golden
from relation_detr_amd import frontend
from relation_detr_amd.frontend import DetrAugment, DetrChoice, ImagePreprocessor, augment, detr_plan, sample_detr_choices, shortest_size, transform_targets
from test_images_host import NEAR_TIE_SHARE, check_normalised, interpolate_error, near_tie, normalised_table, resize64

T = torch.from_numpy
N_CASES = 8


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_augment.npz")


def preset(g15):
    return dict(scales=tuple(g15["preset.scales"].tolist()), max_size=int(g15["preset.max_size"]),
                crop_resize=tuple(g15["preset.crop_resize"].tolist()), crop_range=tuple(g15["preset.crop_range"].tolist()))


def small_augment(g15, **kw):
    return DetrAugment(**preset(g15), eval_min_size=64, eval_max_size=100, **kw)


def case_choice(g15, i) -> DetrChoice:
    flip, crop, min_size, first, ch, cw, top, left = g15[f"c{i}.choice"].tolist()
    return DetrChoice(bool(flip), True, min_size, first, (ch, cw), (top, left)) if crop else DetrChoice(bool(flip), False, min_size)


def case_inputs(g15, i, device="cpu"):
    target = {"boxes": T(g15[f"c{i}.boxes"]).to(device), "labels": T(g15[f"c{i}.labels"]).to(device)}
    return T(g15[f"c{i}.src"]).to(device), target


_REFERENCES = {}


def case_reference(g15, i):
    """(q64, near) of the case's last resize by the float64 filter.  Computed once per case and shared."""
    if i in _REFERENCES:
        return _REFERENCES[i]
    src = g15[f"c{i}.src"]
    flip, crop = g15[f"c{i}.choice"][:2].tolist()
    image = np.ascontiguousarray(src[:, :, ::-1]) if flip else src
    if crop:
        _, _, _, _, ch, cw, top, left = g15[f"c{i}.choice"].tolist()
        v64 = resize64(image, *g15[f"c{i}.first"].tolist())
        q64, near = near_tie(v64, interpolate_error(image, v64))
        window = (slice(None), slice(top, top + ch), slice(left, left + cw))
        assert not near[window].any(), f"case {i}: {int(near[window].sum())} near ties in the crop of the first resize; the case is ill-posed"
        assert np.array_equal(q64[window], g15[f"c{i}.mid"]), f"case {i}: the recorded crop is not the exact first resize"
        image = np.ascontiguousarray(g15[f"c{i}.mid"])
    oh, ow = g15[f"c{i}.final"].tolist()
    v64 = resize64(image, oh, ow)
    q64, near = near_tie(v64, interpolate_error(image, v64))
    assert near.sum() <= NEAR_TIE_SHARE * near.size, f"case {i}: {int(near.sum())} of {near.size} values are near ties; ill-posed"
    _REFERENCES[i] = (q64, near)
    return _REFERENCES[i]


def check_case_batch(g15, cases, batch, prepared, what=""):
    """A batch of fixture cases, from either route: sizes, pixels by the near-tie rule, padding +0, mask, targets bit for bit."""
    finals = [tuple(g15[f"c{i}.final"].tolist()) for i in cases]
    assert batch.image_sizes.tolist() == [list(f) for f in finals], what
    assert batch.original_sizes.tolist() == [list(g15[f"c{i}.src"].shape[1:]) for i in cases], what
    Hp, Wp = frontend.batched_size(finals, 32)
    assert tuple(batch.tensors.shape) == (len(cases), 3, Hp, Wp) and tuple(batch.mask.shape) == (len(cases), Hp, Wp), what
    got, mask = batch.tensors.float().cpu().numpy(), batch.mask.cpu().numpy()
    for k, (i, (oh, ow)) in enumerate(zip(cases, finals)):
        q64, near = case_reference(g15, i)
        check_normalised(got[k, :, :oh, :ow], q64, near, (what, i))
        check_normalised(normalised_table()[np.arange(3).reshape(3, 1, 1), g15[f"c{i}.out"]], q64, near, (what, i, "fixture"))
        pad = got[k].copy()
        pad[:, :oh, :ow] = 0
        assert not pad.view(np.uint32).any(), (what, i, "padding is not +0")
        want_mask = np.ones((Hp, Wp), dtype=bool)
        want_mask[:oh, :ow] = False
        assert np.array_equal(mask[k], want_mask), (what, i)
        expected = frontend.prepare_targets(torch.tensor([[oh, ow]]), [{"boxes": T(g15[f"c{i}.boxes_out"]), "labels": T(g15[f"c{i}.labels_out"])}])[0]
        assert torch.equal(prepared[k]["labels"].cpu(), expected["labels"]), (what, i)
        assert np.array_equal(prepared[k]["boxes"].cpu().numpy().view(np.uint32), expected["boxes"].numpy().view(np.uint32)), (what, i)


# ----------------------------------------------------------------------------------------------------------------- the size rule
def test_shortest_size_is_the_reference_rule(g15):
    table = g15["sizes"].tolist()
    assert len(table) >= 300
    wrong = [r for r in table if shortest_size(r[0], r[1], r[2], None if r[3] < 0 else r[3]) != (r[4], r[5])]
    assert not wrong, wrong[:5]
    assert {(r[2], r[3]) for r in table} >= {(800, 1333), (400, -1), (1200, 2000), (48, 133), (60, -1)}
    # and it is not the float32 rule of EvalResize: the two differ somewhere on this table
    assert any(frontend.resized_size(r[0], r[1], r[2], None if r[3] < 0 else r[3]) != (r[4], r[5]) for r in table)


# ------------------------------------------------------------------------------------------------------------------- the plans
def test_detr_plan_gives_the_reference_sizes_and_windows(g15):
    p = preset(g15)
    seen = set()
    for i in range(N_CASES):
        src, choice = g15[f"c{i}.src"], case_choice(g15, i)
        (flip, first, crop), final = detr_plan(src.shape[1], src.shape[2], choice, p["max_size"], p["crop_range"])
        assert final == tuple(g15[f"c{i}.final"].tolist()) and flip == choice.flip, i
        if choice.crop:
            assert first == tuple(g15[f"c{i}.first"].tolist()), i
            assert crop == tuple(choice.crop_corner) + tuple(choice.crop_size) and g15[f"c{i}.mid"].shape[1:] == crop[2:], i
        else:
            assert first is None and crop is None
        seen.add((choice.flip, choice.crop))
    assert len(seen) == 4                                                         # flip on / off x both branches


def test_detr_plan_refuses_a_crop_outside_the_reference_ranges(g15):
    p = preset(g15)
    h, w = g15["c2.src"].shape[1:]
    good = case_choice(g15, 2)
    rh1, rw1 = shortest_size(h, w, good.first_min_size)
    for bad in (good._replace(crop_size=(p["crop_range"][0] - 1, good.crop_size[1])), good._replace(crop_size=(rh1 + 1, good.crop_size[1])),
                good._replace(crop_size=(good.crop_size[0], p["crop_range"][1] + 1)), good._replace(crop_corner=(-1, 0)),
                good._replace(crop_corner=(rh1 - good.crop_size[0] + 1, 0)), good._replace(crop_corner=(0, rw1 - good.crop_size[1] + 1))):
        with pytest.raises(ValueError, match="detr_plan"):
            detr_plan(h, w, bad, p["max_size"], p["crop_range"])


# ------------------------------------------------------------------------------------------------------------- the torch route
@pytest.mark.parametrize("i", range(N_CASES))
def test_torch_route_reproduces_the_reference_case(g15, i):
    aug = small_augment(g15, fused=False).train()
    image, target = case_inputs(g15, i)
    kept = target["boxes"].clone()
    batch, prepared = aug([image], [target], [case_choice(g15, i)])
    check_case_batch(g15, [i], batch, prepared, "torch route")
    assert torch.equal(target["boxes"], kept)                                      # the input is not overwritten
    assert aug.state_dict() == {} and not list(aug.buffers())


def test_torch_route_reproduces_the_mixed_batch(g15):
    cases = g15["batch.cases"].tolist()
    assert {bool(g15[f"c{i}.choice"][1]) for i in cases} == {False, True}
    aug = small_augment(g15, fused=False).train()
    inputs = [case_inputs(g15, i) for i in cases]
    batch, prepared = aug([im for im, _ in inputs], [t for _, t in inputs], [case_choice(g15, i) for i in cases])
    check_case_batch(g15, cases, batch, prepared, "torch route, batch")


def test_boxes_move_as_the_reference_moves_them(g15):
    p = preset(g15)
    dropped = 0
    for i in range(N_CASES):
        image, target = case_inputs(g15, i)
        plan, final = detr_plan(image.shape[1], image.shape[2], case_choice(g15, i), p["max_size"], p["crop_range"])
        moved = transform_targets([target], [tuple(image.shape[1:])], [plan], [final])[0]
        assert np.array_equal(moved["boxes"].numpy().view(np.uint32), g15[f"c{i}.boxes_out"].view(np.uint32)), i
        assert np.array_equal(moved["labels"].numpy(), g15[f"c{i}.labels_out"]), i
        assert np.array_equal(g15[f"c{i}.labels"][g15[f"c{i}.valid"]], g15[f"c{i}.labels_out"]), i
        dropped += int((~g15[f"c{i}.valid"]).sum())
    assert dropped >= 3 and len(g15["c5.boxes_out"]) == 0                           # sanitising drops boxes; an image may have none


# ------------------------------------------------------------------------------------------------------------------ the sampler
def test_sampler_stays_in_the_reference_ranges_and_follows_its_generator(g15):
    p = preset(g15)
    sizes = [(70, 100), (95, 130), (101, 74), (83, 111)] * 60
    kw = dict(scales=p["scales"], crop_resize=p["crop_resize"], crop_range=p["crop_range"])
    a = sample_detr_choices(sizes, torch.Generator().manual_seed(3), **kw)
    b = sample_detr_choices(sizes, torch.Generator().manual_seed(3), **kw)
    c = sample_detr_choices(sizes, torch.Generator().manual_seed(4), **kw)
    assert a == b and a != c
    lo, hi = p["crop_range"]
    for (h, w), ch in zip(sizes, a):
        assert ch.min_size in p["scales"] and isinstance(ch.flip, bool)
        detr_plan(h, w, ch, p["max_size"], p["crop_range"])                          # inside the reference's ranges, or it raises
        if ch.crop:
            rh1, rw1 = shortest_size(h, w, ch.first_min_size)
            assert ch.first_min_size in p["crop_resize"] and lo <= ch.crop_size[0] <= min(rh1, hi) and lo <= ch.crop_size[1] <= min(rw1, hi)
    assert {(ch.flip, ch.crop) for ch in a} == {(False, False), (False, True), (True, False), (True, True)}
    assert {ch.min_size for ch in a} == set(p["scales"]) and {ch.first_min_size for ch in a if ch.crop} == set(p["crop_resize"])
    assert any(ch.crop and ch.crop_corner[0] == shortest_size(h, w, ch.first_min_size)[0] - ch.crop_size[0] for (h, w), ch in zip(sizes, a))
    flips = sum(ch.flip for ch in a)
    assert 80 <= flips <= 160                                                     # p = 0.5 of 240: 120 +- 5 sigma
    only_resize = sample_detr_choices(sizes, torch.Generator().manual_seed(3), scales=p["scales"], crop_resize=None)
    assert not any(ch.crop for ch in only_resize)                                   # the multiscale preset
    assert not any(ch.flip for ch in sample_detr_choices(sizes[:40], torch.Generator().manual_seed(3), p_flip=0.0, **kw))
    aug = small_augment(g15, fused=False, generator=torch.Generator().manual_seed(3)).train()
    assert aug.sample([torch.empty(3, h, w) for h, w in sizes]) == a


# ------------------------------------------------------------------------------------------------------------------ the module
def test_eval_mode_is_the_image_preprocessor(g15):
    images = [T(g15[f"c{i}.src"]) for i in (0, 4)]
    targets = [{"boxes": T(g15[f"c{i}.boxes_out"]) + 1.0, "labels": T(g15[f"c{i}.labels_out"])} for i in (0, 4)]
    aug = small_augment(g15, fused=False).eval()
    want, want_targets = ImagePreprocessor(64, 100, fused=False).eval()(images, targets)
    got, got_targets = aug(images, targets)
    assert torch.equal(got.tensors, want.tensors) and torch.equal(got.mask, want.mask) and torch.equal(got.image_sizes, want.image_sizes)
    for a, b in zip(got_targets, want_targets):
        assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["labels"], b["labels"])
    aug.train()
    assert aug.training and not aug.eval_preprocessor.training and not aug.batcher.training
    assert relation_detr_amd.DetrAugment(crop_resize=None).crop_resize is None


def test_fused_module_takes_the_torch_route_for_host_tensors(g15):
    image, target = case_inputs(g15, 3)
    aug = small_augment(g15).train()                                               # fused=True
    assert not aug.takes_fused_route([image], [case_choice(g15, 3)])
    batch, prepared = aug([image], [target], [case_choice(g15, 3)])
    check_case_batch(g15, [3], batch, prepared, "fused module, host tensors")
    with pytest.raises(relation_detr_amd._lib.RdetrError, match="not on a ROCm device"):
        aug.forward_fused([image], [target], [case_choice(g15, 3)])


def test_other_layouts_on_the_torch_route(g15):
    image, _ = case_inputs(g15, 2)
    base = small_augment(g15, fused=False).train()([image], None, [case_choice(g15, 2)])[0].tensors
    for dtype in (torch.float32, torch.bfloat16):
        for cl in (False, True):
            t = small_augment(g15, fused=False, dtype=dtype, channels_last=cl).train()([image], None, [case_choice(g15, 2)])[0].tensors
            assert t.dtype == dtype and t.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
            assert torch.equal(t, base.to(dtype))


def test_batch_images_keeps_its_parameters_and_gains_plans():
    params = inspect.signature(frontend.batch_images).parameters
    assert list(params) == ["images", "sizes", "size_divisible", "mean", "std", "normalize", "dtype", "channels_last", "plans"]
    defaults = {n: p.default for n, p in params.items()}
    assert defaults == {"images": inspect.Parameter.empty, "sizes": None, "size_divisible": 32, "mean": (0.485, 0.456, 0.406),
                        "std": (0.229, 0.224, 0.225), "normalize": True, "dtype": torch.float32, "channels_last": False, "plans": None}
    assert params["plans"].kind is inspect.Parameter.KEYWORD_ONLY
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n, p in params.items() if n != "plans")
    for name in ("DetrAugment", "DetrChoice", "detr_plan", "sample_detr_choices", "shortest_size", "transform_targets"):
        assert name in relation_detr_amd.__all__ and getattr(relation_detr_amd, name) is getattr(frontend, name) is getattr(augment, name)


def test_plans_are_checked_before_the_kernel():
    takes = frontend.images._kernel_takes
    fake = torch.empty(3, 70, 100, dtype=torch.uint8, device="meta")

    class OnDevice:                                                                # what _kernel_takes reads of a device image
        def __init__(self, t, dtype=torch.uint8):
            self.t, self.dtype, self.device, self.is_cuda, self.shape = t, dtype, "cuda:0", True, t.shape
        dim, stride = (lambda self: 3), (lambda self, k: self.t.stride(k))
    image = OnDevice(fake)
    real = frontend.images.Tensor
    frontend.images.Tensor = OnDevice
    try:
        ok = [((48, 68), (False, None, None)), ((56, 56), (True, (40, 54), (1, 14, 38, 38))), ((38, 38), (True, (40, 54), (1, 14, 38, 38))),
              ((30, 40), (False, None, (10, 20, 60, 80))), ((40, 54), (True, (40, 54), None))]
        for size, plan in ok:
            assert takes([image], [size], 32, True, [plan]) is None, (size, plan)
        assert takes([image], [(48, 68)], 32, True, None) is None
        bad = [((56, 56), (False, (40, 54), (3, 14, 38, 38)), "outside the resized image"), ((56, 56), (False, (40, 54), (1, 17, 38, 38)), "outside"),
               ((30, 40), (False, None, (11, 20, 60, 80)), "outside the image"), ((56, 56), (False, (8, 54), (0, 0, 8, 38)), "downscale"),
               ((4, 56), (False, (40, 54), (1, 14, 38, 38)), "downscale"), ((8, 100), (True, None, None), "downscale")]
        for size, plan, reason in bad:
            assert reason in takes([image], [size], 32, True, [plan]), (size, plan)
        assert "one per image" in takes([image], [(48, 68)], 32, True, [])
        assert "float images" in takes([OnDevice(fake, torch.float32)], [(56, 56)], 32, True, [(False, (40, 54), (1, 14, 38, 38))])
        assert takes([OnDevice(fake, torch.float32)], [(38, 38)], 32, True, [(False, (40, 54), (1, 14, 38, 38))]) is None
    finally:
        frontend.images.Tensor = real
