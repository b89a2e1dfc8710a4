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
    assert {"backbones.epilogue.frozen_bn_act_backward", "backbones.epilogue.FrozenBNActFunction.backward", "frontend.images.batch_images",
            "frontend.images.ImagePreprocessor.batch_fused"} <= names
    assert {"amp_train.ffn_mixed_backward", "amp_train.ffn_pack_f32", "neck.group_norm_levels_backward", "neck._sine_pos_packed",
            "denoising.cdn_embed_backward", "criterion.assign_match", "criterion._set_loss_torch", "optim.train_step",
            "optim.FusedAdamW._clip_fused", "optim.FusedAdamW._step_fused", "optim.FusedAdamW._prepare"} <= names
    assert not set(shadow.TRAIN_ENTRIES) & shadow.TRAIN_HOST_ONLY
    unclassified = names - set(shadow.TRAIN_ENTRIES) - shadow.TRAIN_HOST_ONLY
    assert not unclassified, f"training-module functions with neither a shadow checker nor a host-only entry: {sorted(unclassified)}"
    stale = (set(shadow.TRAIN_ENTRIES) | shadow.TRAIN_HOST_ONLY) - names
    assert not stale, f"classified names that the training modules no longer define: {sorted(stale)}"
    assert not set(shadow.TRAIN_ENTRIES) & set(shadow.KERNEL_ENTRIES)            # one namespace of op names in the records


def _package_files():
    """{module key: path} of every .py the recursive walk of relation_detr_amd/ visits, and the subpackages it opened.  Keys are the
    dotted path below the package: "ops", "backbones.epilogue", "backbones.__init__", "__init__"."""
    package = os.path.join(ROOT, "relation_detr_amd")
    files, subpackages = {}, set()
    for folder, dirs, names in sorted(os.walk(package)):
        dirs[:] = sorted(d for d in dirs if d != "__pycache__")
        below = os.path.relpath(folder, package)
        parts = [] if below == "." else below.split(os.sep)
        if parts and any(n.endswith(".py") for n in names):
            subpackages.add(".".join(parts))
        for file in sorted(names):
            if file.endswith(".py"):
                files[".".join(parts + [file[:-3]])] = os.path.join(folder, file)
    return files, subpackages


def _resolve(module, level, target):
    """The module key that ``from <level dots><target> import ...`` names inside module ``module`` ("" for the package itself)."""
    base = module.split(".")[:-1]                                   # the module's own package
    base = base[:len(base) - (level - 1)] if level > 1 else base
    return ".".join(base + (target.split(".") if target else []))


def _imports(tree, module, level_limit=2):
    """The relative imports of a module's top level, levels 1 and 2: ``{local name: (module key, original name)}`` for ``from .x import
    name`` and ``from . import x`` alike (the latter: ("", "x") below the package, ("backbones", "epilogue") inside a subpackage)."""
    found = {}
    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and 1 <= node.level <= level_limit:
            for a in node.names:
                found[a.asname or a.name] = (_resolve(module, node.level, node.module), a.name)
    return found


def _package_functions():
    """(module key, "function" or "Class.method") -> (ast node, that module's relative imports, see _imports) for every module-level
    function and every method of a module-level class of every module of relation_detr_amd, subpackages included."""
    out = {}
    for module, path in _package_files()[0].items():
        with open(path) as f:
            tree = ast.parse(f.read())
        imported = _imports(tree, module)
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                out[(module, node.name)] = (node, imported)
            elif isinstance(node, ast.ClassDef):
                for sub in node.body:
                    if isinstance(sub, (ast.FunctionDef, ast.AsyncFunctionDef)):
                        out[(module, f"{node.name}.{sub.name}")] = (sub, imported)
    return out


def _split(key, modules=None):
    """"backbones.epilogue._dense" -> ("backbones.epilogue", "_dense"): the longest module of the package that starts the key."""
    modules = _package_files()[0] if modules is None else modules
    for module in sorted(modules, key=len, reverse=True):
        if key.startswith(module + "."):
            return module, key[len(module) + 1:]
    raise AssertionError(f"{key} names no module of the package")


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


def _refers(node, imported, mod, module, name):
    """Whether the body ``node`` of a function of module ``mod`` refers to function ``name`` of ``module``: the bare name inside the
    module itself or where ``from .module import name`` brought it in (under any local name), or ``<alias>.name`` with ``<alias>`` a
    local name of the module (``from . import ops``, ``from .. import neck as n``)."""
    last = name                                                      # a "Class.method" is never referred to by a bare name
    for sub in ast.walk(node):
        if isinstance(sub, ast.Name):
            if (mod == module and sub.id == last) or imported.get(sub.id) == (module, last):
                return True
        elif isinstance(sub, ast.Attribute) and sub.attr == last and isinstance(sub.value, ast.Name):
            origin = imported.get(sub.value.id)
            if origin is not None and ".".join(p for p in origin if p) == module:
                return True
    return False


def _callers(functions, module, name):
    """Every (module, function) of the package whose body refers to function ``name`` of ``module`` (_refers)."""
    return [(mod, fn) for (mod, fn), (node, imported) in functions.items()
            if (mod, fn) != (module, name) and _refers(node, imported, mod, module, name)]


def test_every_function_that_names_a_launching_symbol_is_a_checked_entry():
    """The hole the symbol test leaves: it knows that every rdetr_* symbol is under the tripwire, not that every Python function
    that calls one is wrapped.  From the source of every module of the package: a function or method that mentions a launching
    symbol is a key of KERNEL_ENTRIES / TRAIN_ENTRIES, or is listed in LAUNCH_INSIDE_ENTRY -- and every caller of a listed function
    is itself a checked entry or listed, so that the tripwire's "inside a checked entry" holds by construction."""
    functions = _package_functions()
    inside = set(shadow.LAUNCH_INSIDE_ENTRY)
    assert {"rowtail.linear_ln_rows", "amp_train.ffn_pack_f32", "ffn_train._pack", "ops._packed_k256"} <= inside
    assert not {k for k in inside if _is_checked_entry(*_split(k))}, "listed as launching inside an entry and as an entry"
    stale = {k for k in inside if _split(k) not in functions}
    assert not stale, f"LAUNCH_INSIDE_ENTRY names functions the package no longer defines: {sorted(stale)}"
    unchecked = {}
    for (module, name), (node, _) in functions.items():
        names = _launching_mentions(node)
        if names and not _is_checked_entry(module, name) and f"{module}.{name}" not in inside:
            unchecked[f"{module}.{name}"] = sorted(names)[:3]
    modules = sorted({_split(k)[0] for k in unchecked})
    assert not unchecked, f"functions of modules {modules} name a launching rdetr_* symbol outside the shadow harness: {unchecked}"
    idle = {k for k in inside if not _launching_mentions(functions[_split(k)][0])
            and not any(f"{m}.{f}" in inside for m, f in _called_listed(functions, k, inside))}
    assert not idle, f"LAUNCH_INSIDE_ENTRY lists functions that neither name a symbol nor call a listed function: {sorted(idle)}"
    loose = {}
    for key in sorted(inside):
        module, name = _split(key)
        bad = [f"{m}.{f}" for m, f in _callers(functions, module, name) if not _is_checked_entry(m, f) and f"{m}.{f}" not in inside]
        if bad:
            loose[key] = bad
    assert not loose, f"functions that launch only inside a checked entry are called from unchecked functions: {loose}"


def _called_listed(functions, key, inside):
    """The listed functions that the listed function ``key`` itself calls (a wrapper around a packer is listed for that)."""
    return [_split(k) for k in inside if k != key and _split(key) in _callers(functions, *_split(k))]


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


# ------------------------------------------------------------------------------------------- the walk itself, and by-name bindings
def test_the_walk_visits_every_file_of_the_package():
    """The guard reads what is on disk: every .py below relation_detr_amd/, found a second way, is a module the walk visited, and the
    walk opened the subpackages (a listing of the package's own folder alone sees none of them)."""
    import pathlib
    files, subpackages = _package_files()
    package = pathlib.Path(ROOT, "relation_detr_amd")
    on_disk = {str(p) for p in package.rglob("*.py") if "__pycache__" not in p.parts}
    assert set(files.values()) == on_disk, sorted(set(files.values()) ^ on_disk)
    assert len(subpackages) >= 2 and {"backbones", "frontend"} <= subpackages, subpackages
    assert {"backbones.epilogue", "backbones.resnet", "frontend.images", "backbones.__init__", "ops", "__init__"} <= set(files)
    modules = {m for m, _ in _package_functions()}
    assert {"backbones.epilogue", "backbones.resnet", "frontend.images"} <= modules


def test_every_module_that_names_a_launching_symbol_is_in_the_harness():
    """Module by module, from the whole source (not only the function bodies): a module that names a launching rdetr_* symbol is ops,
    a module of shadow.TRAIN_MODULES, or the home of a LAUNCH_INSIDE_ENTRY function (rowtail).  _lib is the binding table itself."""
    files, _ = _package_files()
    allowed = {"ops", "_lib"} | set(shadow.TRAIN_MODULES) | {_split(k, files)[0] for k in shadow.LAUNCH_INSIDE_ENTRY}
    naming = {}
    for module, path in files.items():
        with open(path) as f:
            tree = ast.parse(f.read())
        skip = _docstrings(tree) | ({id(tree.body[0].value)} if tree.body and isinstance(tree.body[0], ast.Expr) else set())
        names = {n for n in _launching_mentions(tree) if n in _lib.SIGNATURES or n.endswith("_")}
        names -= {sub.value for sub in ast.walk(tree) if isinstance(sub, ast.Constant) and id(sub) in skip and isinstance(sub.value, str)}
        if names:
            naming[module] = sorted(names)[:3]
    assert {"ops", "backbones.epilogue", "frontend.images", "neck", "rowtail"} <= set(naming), sorted(naming)
    outside = {m: v for m, v in naming.items() if m not in allowed}
    assert not outside, f"modules that name a launching rdetr_* symbol and are not in the shadow harness's module list: {outside}"
    for short in shadow.TRAIN_MODULES:
        assert short in files, f"shadow.TRAIN_MODULES names {short}, which is no module of the package"


def _stub_library(monkeypatch):
    """``_lib.load()`` answers with an object that has every symbol and launches nothing: the harness can be installed without the built
    library and without a device."""
    import types
    stub = types.SimpleNamespace(**{name: (lambda *args: 0) for name in _lib.SIGNATURES})
    monkeypatch.setattr(_lib, "load", lambda: stub)
    return stub


def _reached_entries(functions, module, name, seen=None):
    """The checked entries of ``module`` that its function ``name`` reaches through bare names of that module (a class name stands for
    all its methods), itself included when it is one."""
    seen = set() if seen is None else seen
    if (module, name) in seen or (module, name) not in functions:
        return set()
    seen.add((module, name))
    if _is_checked_entry(module, name):
        return {name}
    node = functions[(module, name)][0]
    used = {sub.id for sub in ast.walk(node) if isinstance(sub, ast.Name)}
    found = set()
    for (mod, fn) in functions:
        if mod == module and fn.split(".")[0] in used:
            found |= _reached_entries(functions, module, fn, seen)
    return found


def test_a_checked_entry_bound_by_name_is_patched_there_too(monkeypatch):
    """``from .epilogue import stem_bn_relu_maxpool`` gives backbones/resnet.py its own reference to the function; a harness that
    patched the defining module alone would leave that call outside itself.  From the source of every module: each ``from .x import
    name`` (levels 1 and 2) of a checked entry must hold the entry's wrapper once ``Shadow`` stands; each one of a host-only function
    of a harness module that reaches entries (``frozen_bn_act``) must hold the function itself, whose own globals then hold the
    wrappers of the entries it reaches."""
    functions = _package_functions()
    files, _ = _package_files()
    harness = {"ops"} | set(shadow.TRAIN_MODULES)
    bindings = []                                                   # (importing module, local name, module, name, entries reached)
    imports = {}
    for module, path in files.items():
        with open(path) as f:
            imports[module] = _imports(ast.parse(f.read()), module)
    for module, imported in imports.items():
        for local, (origin, name) in imported.items():
            while name in imports.get(f"{origin}.__init__", {}):    # a name a subpackage's __init__ re-exports: where that has it from
                origin, name = imports[f"{origin}.__init__"][name]
            if origin in harness and (origin, name) in functions:
                reached = _reached_entries(functions, origin, name)
                if reached:
                    bindings.append((module, local, origin, name, reached))
    found = {(m, l) for m, l, *_ in bindings}
    assert {("backbones.resnet", "stem_bn_relu_maxpool"), ("backbones.resnet", "frozen_bn_act"), ("backbones.__init__", "frozen_bn_act_forward"),
            ("backbones.__init__", "frozen_bn_act_backward"), ("frontend.__init__", "batch_images"), ("__init__", "batch_images")} <= found, found
    _stub_library(monkeypatch)
    sh = shadow.Shadow(monkeypatch)
    assert not sh.errors
    key_of = lambda origin, name: name if origin == "ops" else f"{origin}.{name}"                            # noqa: E731
    wrong = []
    for module, local, origin, name, reached in bindings:
        holder = importlib.import_module("relation_detr_amd" + ("" if module == "__init__" else "." + module.removesuffix(".__init__")))
        bound = getattr(holder, local)
        if _is_checked_entry(origin, name):
            if getattr(bound, "shadow_key", None) != key_of(origin, name):
                wrong.append(f"{module}.{local} is not the wrapper of {key_of(origin, name)}")
            continue
        if hasattr(bound, "shadow_key"):
            wrong.append(f"{module}.{local} is host-only and was wrapped")
        for entry in reached:
            target = bound.__globals__.get(entry.split(".")[0])
            for part in entry.split(".")[1:]:                       # "Class.method": the wrapper sits on the class
                target = getattr(target, part, None)
            if getattr(target, "shadow_key", None) != key_of(origin, entry):
                wrong.append(f"{module}.{local} reaches {origin}.{entry} through a global that is not its wrapper")
    assert not wrong, wrong
    # and the wrappers are one object per entry: the call counter of the entry sees the launches of every binding
    from relation_detr_amd.backbones import epilogue, resnet
    assert resnet.stem_bn_relu_maxpool is epilogue.stem_bn_relu_maxpool and resnet.frozen_bn_act is epilogue.frozen_bn_act
    assert resnet.frozen_bn_act.__globals__["frozen_bn_act_forward"].shadow_key == "backbones.epilogue.frozen_bn_act_forward"


# ------------------------------------------------------------------------------------------------------------ write sets
def _entry_functions():
    """{key: the function} of every checked entry, as the harness finds them."""
    return {key: getattr(owner, attr) for owner, attr, key, entries, _ in shadow.patch_targets() if key in entries}


def test_every_checked_entry_has_a_write_set_and_no_other_key_does():
    entries = set(shadow.KERNEL_ENTRIES) | set(shadow.TRAIN_ENTRIES)
    assert set(shadow.WRITES) == entries, (sorted(entries - set(shadow.WRITES)), sorted(set(shadow.WRITES) - entries))
    assert set(_entry_functions()) == entries
    for key, rule in shadow.WRITES.items():
        assert callable(rule) or (isinstance(rule, tuple) and all(isinstance(n, str) and n and "*" not in n for n in rule)), key
    # callables only where the operands are not arguments: the two launching methods of the optimizer
    assert {k for k, rule in shadow.WRITES.items() if callable(rule)} == {"optim.FusedAdamW._clip_fused", "optim.FusedAdamW._step_fused"}
    assert all(getattr(shadow.TRAIN_ENTRIES[k], "snapshot", None) is not None for k, rule in shadow.WRITES.items() if callable(rule))


def test_every_name_of_a_write_set_is_a_parameter_and_every_out_is_declared():
    functions = _entry_functions()
    for key, rule in shadow.WRITES.items():
        params = inspect.signature(functions[key]).parameters
        if callable(rule):
            assert list(params) [:1] == ["self"], key
            continue
        for name in rule:
            assert name.split(".")[0] in params, f"{key}: `{name}` is no parameter of {list(params)}"
        # a destination: a parameter called out (or ..._out) that may be left out.  The `out` the two attention backwards REQUIRE is
        # the saved forward output, an operand they read: it must come back unchanged and is held to that below
        outs = [n for n, p in params.items() if (n == "out" or n.endswith("_out")) and p.default is None]
        assert set(outs) <= set(rule), f"{key}: takes {outs}, declares {rule}"
        saved = [n for n, p in params.items() if n == "out" and p.default is inspect.Parameter.empty]
        assert not set(saved) & set(rule), f"{key}: the saved forward output is read-only"
    assert {k for k, f in functions.items() if inspect.signature(f).parameters.get("out", None) is not None
            and inspect.signature(f).parameters["out"].default is inspect.Parameter.empty} == {
        "_relation_attention_backward", "attn_rel_train._relation_attention_boxes_backward"}
    declared = {k for k, rule in shadow.WRITES.items() if rule and not callable(rule)}
    assert {"add_layer_norm", "linear_k256", "ffn_k256", "ffn_ln_k256", "linear_ln_k256", "tokens_from_levels", "criterion.assign_match",
            "msda_train_hm.ms_deform_attn_backward_fused_hm", "backbones.epilogue.frozen_bn_act_forward", "bias_softmax_",
            "zero_masked_rows_"} <= declared
    # a function whose name ends in an underscore works in place: its first parameter is declared
    for key, fn in functions.items():
        if key.endswith("_") and not callable(shadow.WRITES[key]):
            assert next(iter(inspect.signature(fn).parameters)) in shadow.WRITES[key], key
