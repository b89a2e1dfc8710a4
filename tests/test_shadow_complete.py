"""CPU-side completeness of the shadow-check harness (tests/shadow.py) and of the switch A/B test: adding an ops entry point, a
function of a training module, a launching rdetr_* symbol or an Options field without a check makes this fail, and so does
dropping a training switch from the training-step test.  Needs neither a GPU nor the built library."""
import dataclasses
import importlib
import inspect
import os

import shadow
import test_gpu_shadow_stack as stack
from relation_detr_amd import _lib, ops, options
from test_gpu_shadow_stack import AB_CASES, COVERED_ELSEWHERE, TRAIN_SWITCHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_ops_function_is_classified():
    names = set(shadow.ops_functions(ops))
    assert not set(shadow.KERNEL_ENTRIES) & shadow.HOST_ONLY
    unclassified = names - set(shadow.KERNEL_ENTRIES) - shadow.HOST_ONLY
    assert not unclassified, f"ops functions with neither a shadow checker nor a host-only entry: {sorted(unclassified)}"
    stale = (set(shadow.KERNEL_ENTRIES) | shadow.HOST_ONLY) - names
    assert not stale, f"classified names that ops no longer defines: {sorted(stale)}"


def test_every_rdetr_symbol_is_under_the_tripwire_or_excluded():
    launching = set(shadow.launching_symbols(_lib.SIGNATURES))
    excluded = set(_lib.SIGNATURES) - launching
    assert excluded == set(shadow.NON_LAUNCHING) | {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert set(shadow.NON_LAUNCHING) <= set(_lib.SIGNATURES)
    assert {"rdetr_msda_forward_fused_resident_bf16", "rdetr_ffn_k256_bf16", "rdetr_linear_pack_k256_bf16"} <= launching


def test_every_options_field_is_switched_in_the_ab_test_or_covered_elsewhere():
    fields = {f.name: f.default for f in dataclasses.fields(options.Options)}
    tested = {name for name, _ in AB_CASES}
    assert not tested & set(COVERED_ELSEWHERE)
    missing = set(fields) - tested - set(COVERED_ELSEWHERE)
    assert not missing, f"Options fields neither A/B-tested nor listed as covered elsewhere: {sorted(missing)}"
    for name, value in AB_CASES:
        assert value != fields[name], (name, value)
    assert ("mask_in_kernel", "always") in AB_CASES and ("mask_in_kernel", "never") in AB_CASES


def test_every_training_module_function_is_classified():
    names = set()
    for short in shadow.TRAIN_MODULES:
        names |= set(shadow.train_functions(importlib.import_module(f"relation_detr_amd.{short}")))
    assert {"ln_train.add_layer_norm_backward", "ffn_train._pack", "msda_train_hm.split_merged_projection"} <= names
    assert not set(shadow.TRAIN_ENTRIES) & shadow.TRAIN_HOST_ONLY
    unclassified = names - set(shadow.TRAIN_ENTRIES) - shadow.TRAIN_HOST_ONLY
    assert not unclassified, f"training-module functions with neither a shadow checker nor a host-only entry: {sorted(unclassified)}"
    stale = (set(shadow.TRAIN_ENTRIES) | shadow.TRAIN_HOST_ONLY) - names
    assert not stale, f"classified names that the training modules no longer define: {sorted(stale)}"
    assert not set(shadow.TRAIN_ENTRIES) & set(shadow.KERNEL_ENTRIES)            # one namespace of op names in the records


def test_covered_elsewhere_names_files_that_exist():
    fields = {f.name for f in dataclasses.fields(options.Options)}
    assert set(COVERED_ELSEWHERE) <= fields
    for field, files in COVERED_ELSEWHERE.items():
        assert isinstance(files, tuple) and len(files) >= 2, field            # the training-step test and the unit tests
        for f in files:
            assert f.startswith("tests/") and os.path.isfile(os.path.join(ROOT, f)), (field, f)
        assert "tests/test_gpu_shadow_stack.py" in files, field


def test_every_covered_elsewhere_switch_is_on_in_the_training_step():
    """The six training-only switches are exactly what is covered elsewhere, and the training-step tests switch on that tuple."""
    defaults = {f.name: f.default for f in dataclasses.fields(options.Options)}
    assert set(TRAIN_SWITCHES) == set(COVERED_ELSEWHERE) and len(set(TRAIN_SWITCHES)) == len(TRAIN_SWITCHES)
    assert {"ffn_train_fused", "ln_train_fused", "msda_train_head_major", "rel_train_fused", "msda_train_fused",
            "attn_train_fused"} <= set(COVERED_ELSEWHERE)
    assert all(defaults[name] is False for name in TRAIN_SWITCHES)             # `on` is the flip
    for test in (stack.test_shadow_all_training_routes_step, stack.test_training_routes_match_defaults_against_fp32):
        assert "TRAIN_SWITCHES" in inspect.getsource(test), test.__name__
    assert "dict.fromkeys(switches, True)" in inspect.getsource(stack._mid_training_step)
