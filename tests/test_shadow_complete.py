"""CPU-side completeness of the shadow-check harness (tests/shadow.py) and of the switch A/B test: adding an ops entry point, a
function of a training module, a launching rdetr_* symbol or an Options field without a check makes this fail, and so does
dropping a training switch from the training-step test.  Needs neither a GPU nor the built library."""
import ast
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
    assert {"amp_train.ffn_mixed_backward", "amp_train.ffn_pack_f32", "neck.group_norm_levels_backward", "neck._sine_pos_packed",
            "denoising.cdn_embed_backward", "criterion.assign_match", "criterion._set_loss_torch", "optim.train_step",
            "optim.FusedAdamW._clip_fused", "optim.FusedAdamW._step_fused", "optim.FusedAdamW._prepare"} <= names
    assert not set(shadow.TRAIN_ENTRIES) & shadow.TRAIN_HOST_ONLY
    unclassified = names - set(shadow.TRAIN_ENTRIES) - shadow.TRAIN_HOST_ONLY
    assert not unclassified, f"training-module functions with neither a shadow checker nor a host-only entry: {sorted(unclassified)}"
    stale = (set(shadow.TRAIN_ENTRIES) | shadow.TRAIN_HOST_ONLY) - names
    assert not stale, f"classified names that the training modules no longer define: {sorted(stale)}"
    assert not set(shadow.TRAIN_ENTRIES) & set(shadow.KERNEL_ENTRIES)            # one namespace of op names in the records


def _package_functions():
    """(module, "function" or "Class.method") -> (ast node, names imported with ``from .x import name`` as {name: x}) for every
    module-level function and every method of a module-level class of relation_detr_amd/*.py."""
    out = {}
    package = os.path.join(ROOT, "relation_detr_amd")
    for file in sorted(os.listdir(package)):
        if not file.endswith(".py"):
            continue
        module = file[:-3]
        with open(os.path.join(package, file)) as f:
            tree = ast.parse(f.read())
        imported = {a.asname or a.name: node.module for node in tree.body if isinstance(node, ast.ImportFrom) and node.level == 1
                    and node.module for a in node.names}
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                out[(module, node.name)] = (node, imported)
            elif isinstance(node, ast.ClassDef):
                for sub in node.body:
                    if isinstance(sub, (ast.FunctionDef, ast.AsyncFunctionDef)):
                        out[(module, f"{node.name}.{sub.name}")] = (sub, imported)
    return out


def _docstrings(node):
    found = set()
    for sub in ast.walk(node):
        if isinstance(sub, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)) and sub.body and isinstance(sub.body[0], ast.Expr) \
                and isinstance(sub.body[0].value, ast.Constant) and isinstance(sub.body[0].value.value, str):
            found.add(id(sub.body[0].value))
    return found


def _launching_mentions(node):
    """The rdetr_* names a function's body mentions: attribute accesses ``.<rdetr_name>`` and string literals that start with
    ``rdetr_`` (a prefix counts: ``getattr(lib, "rdetr_match_cost_" + suffix)``), docstrings and the symbols that launch nothing
    (shadow.NON_LAUNCHING) left out.  The ``*_workspace_bytes`` sizes count: their callers are about to launch."""
    skip, names = _docstrings(node), set()
    for sub in ast.walk(node):
        if isinstance(sub, ast.Attribute) and sub.attr.startswith("rdetr_"):
            names.add(sub.attr)
        elif isinstance(sub, ast.Constant) and isinstance(sub.value, str) and sub.value.startswith("rdetr_") and id(sub) not in skip:
            names.add(sub.value)
    return names - set(shadow.NON_LAUNCHING)


def _is_checked_entry(module, name):
    return (name in shadow.KERNEL_ENTRIES) if module == "ops" else (f"{module}.{name}" in shadow.TRAIN_ENTRIES)


def _callers(functions, module, name):
    """Every (module, function) of the package whose body refers to function ``name`` of ``module``: the bare name inside the module
    itself or where ``from .module import name`` brought it in, or ``module.name`` anywhere."""
    found = []
    for (mod, fn), (node, imported) in functions.items():
        if (mod, fn) == (module, name):
            continue
        for sub in ast.walk(node):
            bare = isinstance(sub, ast.Name) and sub.id == name and (mod == module or imported.get(name) == module)
            dotted = isinstance(sub, ast.Attribute) and sub.attr == name and isinstance(sub.value, ast.Name) and sub.value.id == module
            if bare or dotted:
                found.append((mod, fn))
                break
    return found


def test_every_function_that_names_a_launching_symbol_is_a_checked_entry():
    """The hole the symbol test leaves: it knows that every rdetr_* symbol is under the tripwire, not that every Python function
    that calls one is wrapped.  From the source of every module of the package: a function or method that mentions a launching
    symbol is a key of KERNEL_ENTRIES / TRAIN_ENTRIES, or is listed in LAUNCH_INSIDE_ENTRY -- and every caller of a listed function
    is itself a checked entry or listed, so that the tripwire's "inside a checked entry" holds by construction."""
    functions = _package_functions()
    inside = set(shadow.LAUNCH_INSIDE_ENTRY)
    assert {"rowtail.linear_ln_rows", "amp_train.ffn_pack_f32", "ffn_train._pack", "ops._packed_k256"} <= inside
    assert not {k for k in inside if _is_checked_entry(*k.split(".", 1))}, "listed as launching inside an entry and as an entry"
    stale = {k for k in inside if tuple(k.split(".", 1)) not in functions}
    assert not stale, f"LAUNCH_INSIDE_ENTRY names functions the package no longer defines: {sorted(stale)}"
    unchecked = {}
    for (module, name), (node, _) in functions.items():
        names = _launching_mentions(node)
        if names and not _is_checked_entry(module, name) and f"{module}.{name}" not in inside:
            unchecked[f"{module}.{name}"] = sorted(names)[:3]
    modules = sorted({k.split(".", 1)[0] for k in unchecked})
    assert not unchecked, f"functions of modules {modules} name a launching rdetr_* symbol outside the shadow harness: {unchecked}"
    idle = {k for k in inside if not _launching_mentions(functions[tuple(k.split(".", 1))][0])
            and not any(f"{m}.{f}" in inside for m, f in _called_listed(functions, k, inside))}
    assert not idle, f"LAUNCH_INSIDE_ENTRY lists functions that neither name a symbol nor call a listed function: {sorted(idle)}"
    loose = {}
    for key in sorted(inside):
        module, name = key.split(".", 1)
        bad = [f"{m}.{f}" for m, f in _callers(functions, module, name) if not _is_checked_entry(m, f) and f"{m}.{f}" not in inside]
        if bad:
            loose[key] = bad
    assert not loose, f"functions that launch only inside a checked entry are called from unchecked functions: {loose}"


def _called_listed(functions, key, inside):
    """The listed functions that the listed function ``key`` itself calls (a wrapper around a packer is listed for that)."""
    return [tuple(k.split(".", 1)) for k in inside if k != key and tuple(key.split(".", 1)) in _callers(functions, *k.split(".", 1))]


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
