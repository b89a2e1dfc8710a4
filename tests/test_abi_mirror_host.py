"""The ctypes binding (relation_detr_amd/_lib.py) against the C header (include/relation_detr_amd.h), type by type, for every symbol.

The other host tests compare names (and argument counts for a few symbols).  A ``c_int`` where the header says ``long long`` passes
a row stride with undefined upper bits and no name comparison notices, so here every prototype of the header is parsed, its
parameter types are mapped to ctypes -- any pointer -> ``c_void_p``; ``int``, ``float``, ``long long`` / ``int64_t``, ``unsigned long
long`` / ``uint64_t`` -> their ctypes equivalents -- and compared in order with ``_lib.SIGNATURES[name]``, the return type with the
``restype`` that ``_lib.load()`` sets.  A C type the table does not know fails the test; it is never skipped.  Needs neither a GPU
nor the built library (``load()`` runs against a stand-in for the shared object)."""
import ctypes
import os
import re

import pytest

from relation_detr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong, "int64_t": ctypes.c_longlong,
           "unsigned long long": ctypes.c_ulonglong, "uint64_t": ctypes.c_ulonglong}
RETURNS = dict(SCALARS, **{"const char *": ctypes.c_char_p})
PROTOTYPE = re.compile(r"\s*((?:const\s+)?[A-Za-z_][\w\s]*?[\s\*]+)(rdetr_\w+)\s*\(([^()]*)\)\s*", re.S)


def statements(text):
    """The header's statements at file scope: comments, preprocessor lines, the ``extern "C"`` wrapper and brace blocks removed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    while re.search(r"\{[^{}]*\}", text):
        text = re.sub(r"\{[^{}]*\}", " ", text)
    return [s for s in text.replace("}", ";").split(";") if s.strip()]


def c_type(declaration, table, what):
    """'const uint16_t *x' -> c_void_p; 'long long ldx' -> c_longlong; a type the table lacks -> an error."""
    d = " ".join(declaration.replace("*", " * ").split())
    if "*" in d and table is SCALARS:
        return ctypes.c_void_p
    if d in table:                                             # a return type, or an unnamed parameter
        return table[d]
    head, _, name = d.rpartition(" ")
    if table is SCALARS and head in table and re.fullmatch(r"[A-Za-z_]\w*", name):
        return table[head]
    raise AssertionError(f"{what}: no ctypes mapping for the C type of `{declaration.strip()}`")


def prototypes(text):
    """-> {name: (restype, [argtypes])} of every ``rdetr_*`` function the header declares."""
    found = {}
    for statement in statements(text):
        m = PROTOTYPE.fullmatch(statement)
        if m is None:
            assert not re.search(r"\brdetr_\w+\s*\(", statement), f"a declaration the parser cannot read: `{' '.join(statement.split())}`"
            continue
        ret, name, params = m.groups()
        params = " ".join(params.split())
        args = [] if params in ("", "void") else [c_type(p, SCALARS, name) for p in params.split(",")]
        assert name not in found, f"{name} is declared twice"
        found[name] = (c_type(ret, RETURNS, name + " (return type)"), args)
    return found


@pytest.fixture
def loaded(monkeypatch):
    """``_lib.load()`` run on a stand-in for the shared object -> {name: the function object it configured}."""
    class Function:
        argtypes = restype = None

        def __call__(self, *args):
            return 3                                           # rdetr_abi_version()

    class Library:
        def __init__(self, path):
            self.functions = {}

        def __getattr__(self, name):
            if not name.startswith("rdetr_"):
                raise AttributeError(name)
            return self.functions.setdefault(name, Function())
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", Library)
    monkeypatch.setattr(_lib.os.path, "exists", lambda path: True)
    return _lib.load().functions


def test_every_prototype_of_the_header_is_mirrored_type_by_type(loaded):
    with open(os.path.join(ROOT, "include", "relation_detr_amd.h")) as f:
        header = prototypes(f.read())
    assert set(header) == set(_lib.SIGNATURES), (sorted(set(header) - set(_lib.SIGNATURES)), sorted(set(_lib.SIGNATURES) - set(header)))
    assert len(header) >= 111 and set(loaded) == set(header)
    wrong = []
    for name, (restype, args) in sorted(header.items()):
        bound = list(_lib.SIGNATURES[name])
        if len(bound) != len(args):
            wrong.append(f"{name}: {len(args)} parameters in the header, {len(bound)} in the binding")
            continue
        wrong += [f"{name}: parameter {i} is {want.__name__} in the header, {got.__name__} in the binding"
                  for i, (want, got) in enumerate(zip(args, bound)) if want is not got]
        if loaded[name].argtypes != bound:
            wrong.append(f"{name}: load() set other argtypes than SIGNATURES")
        if loaded[name].restype is not restype:
            wrong.append(f"{name}: returns {restype.__name__} in the header, load() sets {getattr(loaded[name].restype, '__name__', None)}")
    assert not wrong, "\n".join(wrong)
    # the comparison saw the types that matter: strides as long long, counts as unsigned long long, sizes returned as long long
    assert any(ctypes.c_longlong in a for _, a in header.values()) and any(ctypes.c_ulonglong in a for _, a in header.values())
    assert header["rdetr_msda_backward_det_workspace_bytes"][0] is ctypes.c_longlong and header["rdetr_status_string"][0] is ctypes.c_char_p


def test_the_parser_reads_c_as_written():
    text = """
    /* int rdetr_in_a_comment(int a); */
    int rdetr_a(void);   // int rdetr_in_a_line_comment(float x);
    const char *rdetr_b(int status);
    long long rdetr_c(const uint16_t *x, long long ldx, const int64_t* shapes, int64_t n, unsigned long long seed,
                      uint64_t key, float eps, void *stream, const rdetr_image_desc *images, float
                      split_over_lines);
    typedef struct rdetr_s { int rdetr_like_a_field; } rdetr_s;
    """
    got = prototypes(text)
    vp, ll, ull = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong
    assert got == {"rdetr_a": (ctypes.c_int, []), "rdetr_b": (ctypes.c_char_p, [ctypes.c_int]),
                   "rdetr_c": (ll, [vp, ll, vp, ll, ull, ull, ctypes.c_float, vp, vp, ctypes.c_float])}


@pytest.mark.parametrize("declaration", ["int rdetr_x(size_t n);", "int rdetr_x(double eps);", "int rdetr_x(unsigned n);",
                                         "int rdetr_x(rdetr_image_desc by_value);", "short rdetr_x(int n);", "void *rdetr_x(int n);"])
def test_an_unknown_c_type_fails(declaration):
    with pytest.raises(AssertionError, match="no ctypes mapping"):
        prototypes(declaration)


def test_a_narrowed_stride_is_caught(loaded, monkeypatch):
    """What the comparison is for: ``long long ld`` bound as ``c_int``."""
    with open(os.path.join(ROOT, "include", "relation_detr_amd.h")) as f:
        header = prototypes(f.read())
    name = "rdetr_value_to_head_major_bf16"
    at = header[name][1].index(ctypes.c_longlong)
    narrowed = list(_lib.SIGNATURES[name])
    assert narrowed[at] is ctypes.c_longlong
    narrowed[at] = ctypes.c_int
    assert [i for i, (want, got) in enumerate(zip(header[name][1], narrowed)) if want is not got] == [at]
