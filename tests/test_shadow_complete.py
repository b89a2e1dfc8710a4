"""CPU-side completeness of the shadow-check harness (tests/shadow.py) and of the switch A/B test: adding an ops entry point, a
launching rdetr_* symbol or an Options field without a check makes this fail.  Needs neither a GPU nor the built library."""
import dataclasses

import shadow
from relation_detr_amd import _lib, ops, options
from test_gpu_shadow_stack import AB_CASES, COVERED_ELSEWHERE


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
