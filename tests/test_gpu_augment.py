"""GPU checks of the training augmentation's kernel route (csrc/images.hip: ``rdetr_augment_image_batch``; ``batch_images(plans=...)``;
frontend/augment.py).  ``shadow.chk_batch_images`` restates the plain call only, so these tests check the augmented calls themselves.

Three kinds of comparison:
  identities      free of ties, so bit for bit, against the plain call (which tests/test_gpu_images.py holds to float64): a flip equals
                  the plain call on ``x.flip(-1)``; a window of a resize equals the same crop of the plain call's result; a resize,
                  crop, resize chain equals the plain call on the uint8 crop that the window route exposes through the normalise
                  table; an image in a batch equals the same image alone
  fixture cases   the reference's recorded cases (tests/golden/g15_augment.npz) by the near-tie rule with the float64 filter, the zero-tie
                  precondition of the first resize asserted first (test_augment_host.case_reference)
  memory          padding +0 and mask True on poisoned memory, no write outside the batch, the mask and the call's scratch (guard bands),
                  the sources bit-identical afterwards
Tiles are 16 x 64; the shapes are the smallest that put a flip, a window and the uint8 scratch on each side of a tile edge."""
import numpy as np
import pytest
import torch

import guard
from relation_detr_amd import _lib, frontend
from relation_detr_amd.frontend import DetrChoice, batch_images
from test_augment_host import N_CASES, case_choice, case_inputs, case_reference, check_case_batch, g15, small_augment  # noqa: F401
from test_gpu_images import random_images
from test_images_host import normalised_table, tiny_detector

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
LAYOUTS = [(F32, False), (BF16, False), (F32, True), (BF16, True)]


def same(a, b, what=""):
    assert a.tensors.dtype == b.tensors.dtype and a.tensors.shape == b.tensors.shape, what
    assert torch.equal(a.tensors.view(torch.int32 if a.tensors.dtype == F32 else torch.int16),
                       b.tensors.view(torch.int32 if b.tensors.dtype == F32 else torch.int16)), (what, "tensors")
    assert torch.equal(a.mask, b.mask) and torch.equal(a.image_sizes, b.image_sizes), (what, "mask")


def crop_of(batch, top, left, ch, cw, index=0):
    return batch.tensors[index, :, top:top + ch, left:left + cw]


# -------------------------------------------------------------------------------------------------------------- tie-free identities
@pytest.mark.parametrize("src_dtype", (U8, F32))
def test_flip_equals_the_plain_call_on_the_flipped_image(src_dtype):
    # widths below 64 and no multiple of 16, one lane, one tile and a half, a copy (no resize), an upscale and two downscales
    originals = [(37, 67), (50, 91), (64, 33), (9, 1), (21, 45), (131, 155)]
    sizes = [(45, 83), (31, 57), (64, 33), (13, 3), (21, 45), (32, 33)]
    sources = [s.to(DEV) for s in random_images(originals, src_dtype, 31)]
    flipped = [s.flip(-1).contiguous() for s in sources]
    for dtype, cl in LAYOUTS:
        got = batch_images(sources, sizes, dtype=dtype, channels_last=cl, plans=[(True, None, None)] * len(sources))
        want = batch_images(flipped, sizes, dtype=dtype, channels_last=cl)
        same(got, want, (src_dtype, dtype, cl))
        assert got.original_sizes.tolist() == [list(s) for s in originals]
    unflipped = batch_images(sources, sizes, plans=[(False, None, None)] * len(sources))
    same(unflipped, batch_images(sources, sizes), "no flip")
    same(batch_images(sources, sizes, plans=[None] * len(sources)), unflipped, "plan None")
    assert not torch.equal(unflipped.tensors, batch_images(sources, sizes, plans=[(True, None, None)] * len(sources)).tensors)


# (source, first resize, window (top, left, ch, cw)): odd corners; the last row and column; inside one tile; across four tiles
WINDOWS = [((70, 100), (53, 150), (3, 7, 11, 40)), ((70, 100), (53, 150), (37, 81, 16, 69)), ((70, 100), (53, 150), (9, 57, 13, 21)),
           ((70, 100), (53, 150), (5, 9, 33, 70)), ((90, 71), (41, 31), (1, 1, 40, 30)), ((131, 155), (32, 33), (5, 3, 21, 29)), ((40, 60), (40, 60), (7, 13, 25, 41))]


@pytest.mark.parametrize("src_dtype", (U8, F32))
@pytest.mark.parametrize("flip", (False, True))
def test_window_equals_the_crop_of_the_plain_call(src_dtype, flip):
    sources = [s.to(DEV) for s in random_images([w[0] for w in WINDOWS], src_dtype, 37)]
    seen = [s.flip(-1).contiguous() if flip else s for s in sources]
    plans = [(flip, first, window) for _, first, window in WINDOWS]
    sizes = [window[2:] for _, _, window in WINDOWS]
    for dtype, cl in LAYOUTS:
        got = batch_images(sources, sizes, dtype=dtype, channels_last=cl, plans=plans)
        whole = batch_images(seen, [first for _, first, _ in WINDOWS], dtype=dtype, channels_last=cl)
        for k, (_, _, (top, left, ch, cw)) in enumerate(WINDOWS):
            assert torch.equal(crop_of(got, 0, 0, ch, cw, k), crop_of(whole, top, left, ch, cw, k)), (src_dtype, flip, dtype, cl, k)
            pad = got.tensors[k].float().clone()
            pad[:, :ch, :cw] = 0
            assert not pad.cpu().numpy().view(np.uint32).any() and not got.mask[k, :ch, :cw].any()
            assert got.mask[k, ch:].all() and got.mask[k, :, cw:].all()


def exposed_bytes(batch, ch, cw, index=0):
    """The uint8 values behind a normalised fp32 batch of uint8 sources: the table is strictly increasing per channel."""
    table = normalised_table()
    got = batch.tensors[index, :, :ch, :cw].cpu().numpy()
    q = np.stack([np.searchsorted(table[c], got[c]) for c in range(3)])
    assert np.array_equal(table[np.arange(3).reshape(3, 1, 1), q], got)
    return torch.from_numpy(q.astype(np.uint8))


# (source, first, window, final): crop widths 40, 69 and 21 leave 8, 5 and 5 columns of the last 16-byte piece of a scratch row
CHAINS = [((70, 100), (53, 150), (3, 7, 11, 40), (17, 61)), ((70, 100), (53, 150), (37, 81, 16, 69), (13, 50)),
          ((70, 100), (53, 150), (9, 57, 13, 21), (29, 47)), ((40, 60), (40, 60), (7, 13, 25, 41), (33, 54))]


@pytest.mark.parametrize("flip", (False, True))
def test_chain_equals_the_plain_call_on_the_exposed_crop(flip):
    sources = [s.to(DEV) for s in random_images([c[0] for c in CHAINS], U8, 41)]
    exposed = batch_images(sources, [c[2][2:] for c in CHAINS], plans=[(flip, c[1], c[2]) for c in CHAINS])
    crops = [exposed_bytes(exposed, c[2][2], c[2][3], k).to(DEV) for k, c in enumerate(CHAINS)]
    finals = [c[3] for c in CHAINS]
    for dtype, cl in LAYOUTS:
        got = batch_images(sources, finals, dtype=dtype, channels_last=cl, plans=[(flip, c[1], c[2]) for c in CHAINS])
        same(got, batch_images(crops, finals, dtype=dtype, channels_last=cl), (flip, dtype, cl))
    # a first resize with no crop is the whole window; a crop with no first resize is a view of the (flipped) source
    k, (_, first, _, final) = 0, CHAINS[0]
    whole = exposed_bytes(batch_images(sources[:1], [first], plans=[(flip, first, None)]), *first).to(DEV)
    same(batch_images(sources[:1], [final], plans=[(flip, first, None)]), batch_images([whole], [final]), "first, no crop")
    top, left, ch, cw = 5, 9, 33, 47
    seen = sources[0].flip(-1) if flip else sources[0]
    same(batch_images(sources[:1], [final], plans=[(flip, None, (top, left, ch, cw))]),
         batch_images([seen[:, top:top + ch, left:left + cw].contiguous()], [final]), "crop, no first")


def test_copy_tile_with_flip_and_window():
    for src_dtype in (U8, F32):
        source = random_images([(40, 150)], src_dtype, 43)[0].to(DEV)
        for top, left, ch, cw in ((0, 0, 40, 150), (7, 13, 25, 41), (1, 81, 39, 69), (3, 5, 16, 64), (0, 149, 40, 1)):
            for flip in (False, True):
                seen = source.flip(-1) if flip else source
                want = batch_images([seen[:, top:top + ch, left:left + cw].contiguous()], [(ch, cw)])
                same(batch_images([source], [(ch, cw)], plans=[(flip, (40, 150), (top, left, ch, cw))]), want, (src_dtype, top, left, flip))


def test_source_that_is_a_view_with_a_longer_row_stride():
    big = random_images([(90, 150)], U8, 47)[0].to(DEV)
    view = big[:, 7:80, 13:118]
    assert not view.is_contiguous() and view.stride(1) == 150
    plans = [(True, None, None), (True, (60, 86), (3, 5, 41, 70)), (False, (60, 86), (3, 5, 41, 70)), (True, None, (5, 9, 33, 47))]
    sizes = [(57, 83), (50, 85), (41, 70), (40, 57)]
    same(batch_images([view] * 4, sizes, plans=plans), batch_images([view.contiguous()] * 4, sizes, plans=plans), "view")
    assert torch.equal(big[:, 7:80, 13:118], view)


# -------------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_first_resize_alone(g15):
    """A crop case with the second resize left out: the normalise table exposes the uint8 crop, which the fixture records exactly."""
    for i in range(N_CASES):
        choice = case_choice(g15, i)
        if not choice.crop:
            continue
        case_reference(g15, i)                                                      # the zero-tie precondition, or ill-posed
        image, _ = case_inputs(g15, i, DEV)
        plan = (choice.flip, tuple(g15[f"c{i}.first"].tolist()), tuple(choice.crop_corner) + tuple(choice.crop_size))
        batch = batch_images([image], [choice.crop_size], plans=[plan])
        assert np.array_equal(exposed_bytes(batch, *choice.crop_size).numpy(), g15[f"c{i}.mid"]), i


@pytest.mark.parametrize("i", range(N_CASES))
def test_fixture_case_through_the_fused_route(g15, i):
    aug = small_augment(g15).train()
    image, target = case_inputs(g15, i, DEV)
    assert aug.takes_fused_route([image], [case_choice(g15, i)])
    batch, prepared = aug([image], [target], [case_choice(g15, i)])
    assert batch.tensors.is_cuda and prepared[0]["boxes"].is_cuda
    check_case_batch(g15, [i], batch, prepared, "fused route")


def test_fixture_mixed_batch_every_layout(g15):
    cases = g15["batch.cases"].tolist()
    inputs = [case_inputs(g15, i, DEV) for i in cases]
    images, targets, choices = [im for im, _ in inputs], [t for _, t in inputs], [case_choice(g15, i) for i in cases]
    base, prepared = small_augment(g15).train()(images, targets, choices)
    check_case_batch(g15, cases, base, prepared, "fused route, batch")
    for dtype, cl in LAYOUTS[1:]:
        other, _ = small_augment(g15, dtype=dtype, channels_last=cl).train()(images, targets, choices)
        assert other.tensors.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        assert torch.equal(other.tensors, base.tensors.to(dtype)) and torch.equal(other.mask, base.mask)


# --------------------------------------------------------------------------------------------------------------- batches and limits
def test_seventeen_images_make_two_launches_per_stage():
    B = frontend.MAX_IMAGES + 1
    originals = [(40 + i, 61 + 2 * i) for i in range(B)]
    plans = [(bool(i % 2), (30 + i, 50 + i), (i % 5, i % 7, 20 + i % 3, 33 + i)) for i in range(B)]
    sizes = [(23 + i, 37 + i) for i in range(B)]
    sources = [s.to(DEV) for s in random_images(originals, U8, 53)]
    batch = batch_images(sources, sizes, plans=plans)
    for k in (0, 7, 15, 16):
        one = batch_images(sources[k:k + 1], sizes[k:k + 1], plans=plans[k:k + 1])
        assert torch.equal(one.tensors[0, :, :sizes[k][0], :sizes[k][1]], batch.tensors[k, :, :sizes[k][0], :sizes[k][1]]), k
        assert not batch.mask[k, :sizes[k][0], :sizes[k][1]].any() and batch.mask[k, sizes[k][0]:].all() and batch.mask[k, :, sizes[k][1]:].all()


def test_batch_mixing_no_plan_resize_only_and_crop_plans():
    originals = [(50, 91), (70, 100), (64, 33), (70, 100), (45, 83)]
    plans = [None, (True, None, None), (False, None, (3, 1, 50, 30)), (True, (53, 150), (37, 81, 16, 69)), (False, (40, 74), (0, 0, 40, 74))]
    sizes = [(31, 57), (83, 119), (61, 37), (13, 50), (40, 74)]
    sources = [s.to(DEV) for s in random_images(originals, U8, 59)]
    batch = batch_images(sources, sizes, plans=plans)
    same(batch_images(sources[:1], sizes[:1], plans=[None]), batch_images(sources[:1], sizes[:1]), "plan None")
    for k, (oh, ow) in enumerate(sizes):
        one = batch_images(sources[k:k + 1], sizes[k:k + 1], plans=plans[k:k + 1])
        assert torch.equal(one.tensors[0, :, :oh, :ow], batch.tensors[k, :, :oh, :ow]), k


def test_beyond_the_downscale_limit(g15):
    source = random_images([(400, 90)], U8, 3)[0].to(DEV)
    with pytest.raises(_lib.RdetrError, match="downscale"):
        batch_images([source], [(50, 11)], plans=[(True, None, None)])                 # 8.2 x down in width
    with pytest.raises(_lib.RdetrError, match="downscale"):
        batch_images([source], [(38, 38)], plans=[(False, (49, 11), (0, 0, 38, 11))])
    with pytest.raises(_lib.RdetrError, match="float images"):
        batch_images([source.float() / 255], [(38, 38)], plans=[(False, (200, 45), (0, 0, 40, 40))])
    with pytest.raises(_lib.RdetrError, match="outside"):
        batch_images([source], [(38, 38)], plans=[(False, (200, 45), (170, 0, 38, 38))])
    aug = frontend.DetrAugment(scales=(11,), max_size=50, crop_resize=None).train()
    choice = [DetrChoice(True, False, 11)]
    assert 90 > frontend.MAX_DOWNSCALE * frontend.detr_plan(400, 90, choice[0], 50)[1][1] and not aug.takes_fused_route([source], choice)
    got, _ = aug([source], None, choice)
    want, _ = frontend.DetrAugment(scales=(11,), max_size=50, crop_resize=None, fused=False).train()([source], None, choice)
    assert torch.equal(got.tensors, want.tensors) and torch.equal(got.mask, want.mask)
    # the C entry refuses what the Python check refuses
    import ctypes
    d = frontend.images._WindowDesc(source.data_ptr(), 90, 36000, 400, 90, 1, 50, 11, 0, 0, 50, 11, None, 0, 0)
    out, mask = torch.empty(1, 3, 64, 32, device=DEV), torch.empty(1, 64, 32, dtype=torch.bool, device=DEV)
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    call = _lib.load().rdetr_augment_image_batch
    table = (frontend.images._WindowDesc * 1)(d)
    assert call(table, 1, 1, 0, 64, 32, mean, std, 1, 0, 0, out.data_ptr(), mask.data_ptr(), None) == -2
    d.rw, d.ow, d.left = 12, 11, 2
    assert call((frontend.images._WindowDesc * 1)(d), 1, 1, 0, 64, 32, mean, std, 1, 0, 0, out.data_ptr(), mask.data_ptr(), None) == -1
    d.left = 1
    assert call((frontend.images._WindowDesc * 1)(d), 1, 1, 1, 0, 0, None, None, 0, 0, 0, None, None, None) == -1      # U8 mode, no dst


# ------------------------------------------------------------------------------------------------------------------------ memory
def test_writes_stay_inside_the_batch_the_mask_and_the_scratch(monkeypatch):
    """Allocations poisoned (0x42) and between guard bands: the padding is still +0 with mask True, no band is touched -- the scratch
    rows of whole 16-byte pieces included -- and the sources come back bit for bit."""
    kept = random_images([(70, 100), (70, 100), (40, 60), (50, 91)], U8, 61)
    plans = [(True, (53, 150), (37, 81, 16, 69)), (False, (53, 150), (9, 57, 13, 21)), (True, (40, 60), (7, 13, 25, 41)), (True, None, None)]
    sizes = [(13, 50), (29, 47), (33, 54), (31, 57)]
    want = batch_images([s.to(DEV) for s in kept], sizes, plans=plans)
    torch.cuda.synchronize()
    g = guard.guard(monkeypatch)
    sources = [torch.empty(s.shape, dtype=U8, device=DEV).copy_(s) for s in kept]
    for dtype, cl in ((F32, False), (BF16, True)):
        before = len(g.allocations)
        got = batch_images(sources, sizes, dtype=dtype, channels_last=cl, plans=plans)
        torch.cuda.synchronize()
        assert len(g.allocations) - before == 3                                      # the batch, the mask and one scratch allocation
        assert g.check() == []
        assert torch.equal(got.tensors, want.tensors.to(dtype)) and torch.equal(got.mask, want.mask)
        for k, (oh, ow) in enumerate(sizes):
            pad = got.tensors[k].float().clone()
            pad[:, :oh, :ow] = 0
            assert not pad.cpu().numpy().view(np.uint32).any() and got.mask[k, oh:].all() and got.mask[k, :, ow:].all()
    for s, k in zip(sources, kept):
        assert torch.equal(s.cpu(), k)


def test_orders_after_work_on_its_stream():
    old, new = random_images([(70, 100), (70, 100)], U8, 67)
    plans, sizes = [(True, (53, 150), (37, 81, 16, 69))], [(13, 50)]
    want = batch_images([new.to(DEV)], sizes, plans=plans)
    source, fresh = old.to(DEV), new.to(DEV)
    a = torch.randn(1024, 1024, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(8):                                                           # work in front of the copy on the side stream
            a = a @ a * 1e-3
        source.copy_(fresh, non_blocking=True)
        got = batch_images([source], sizes, plans=plans)
    side.synchronize()
    same(got, want, "side stream")


# -------------------------------------------------------------------------------------------------------------------- end to end
def test_detector_trains_from_decoded_images(g15):
    from relation_detr_amd.optim import FusedAdamW, relation_param_groups, train_step
    cases = g15["batch.cases"].tolist()
    inputs = [case_inputs(g15, i, DEV) for i in cases]
    images, targets, choices = [im for im, _ in inputs], [t for _, t in inputs], [case_choice(g15, i) for i in cases]
    model = tiny_detector(DEV, True, pre=small_augment(g15)).train()
    assert isinstance(model.preprocessor, frontend.DetrAugment) and model.preprocessor.takes_fused_route(images, choices)
    fused_batch, fused_targets = model.preprocessor(images, targets, choices)
    torch_batch, torch_targets = small_augment(g15, fused=False).train()(images, targets, choices)
    check_case_batch(g15, cases, fused_batch, fused_targets, "detector, fused route")
    check_case_batch(g15, cases, torch_batch, torch_targets, "detector, torch route")
    assert torch.equal(fused_batch.mask, torch_batch.mask) and torch.equal(fused_batch.image_sizes, torch_batch.image_sizes)
    for a, b in zip(fused_targets, torch_targets):
        assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["labels"], b["labels"])

    class Fixed(torch.nn.Module):                                                     # the recorded choices instead of fresh draws
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, images, targets=None):
            return self.inner(images, targets, choices)
    model.preprocessor = Fixed(model.preprocessor).train()
    opt = FusedAdamW(relation_param_groups(model, 1e-3), lr=1e-3, weight_decay=1e-4, fused=True)
    head = lambda batch, _, tgts, noise=None: model(batch, tgts, noise)             # noqa: E731
    losses, norm = train_step(head, opt, images, None, None, targets, max_norm=0.1)
    torch.cuda.synchronize()
    assert len(losses) == 33 and all(bool(torch.isfinite(v)) for v in losses.values()) and bool(torch.isfinite(norm))
    # and with choices drawn by the module itself: the front end alone, the network behind it has run
    drawn = small_augment(g15, generator=torch.Generator().manual_seed(5)).train()
    batch, prepared = drawn(images, targets)
    again, _ = small_augment(g15, generator=torch.Generator().manual_seed(5)).train()(images, targets)
    assert torch.equal(batch.tensors, again.tensors) and torch.equal(batch.image_sizes, again.image_sizes) and len(prepared) == len(images)
    assert not batch.mask[:, 0, 0].any() and torch.isfinite(batch.tensors).all()
