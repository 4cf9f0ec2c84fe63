"""CPU: the C-ABI library loads and exports every symbol include/lkamd.h declares."""
import ctypes

import pytest


def test_library_exports_every_declared_symbol():
    from lkpy_amd import _native

    lib = _native.load(build_if_missing=True)
    names = _native.declared_symbols()
    assert len(names) >= 20
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_version_padding_and_errors_without_gpu():
    from lkpy_amd import _native

    lib = _native.load(build_if_missing=True)
    assert b"gfx950" in lib.lk_version()
    assert [lib.lk_padded_dim(k) for k in (1, 16, 17, 25, 64, 65, 128, 200, 256)] == [
        16, 16, 32, 32, 64, 128, 128, 256, 256]  # fmt: skip
    assert lib.lk_padded_dim(0) == 0 and lib.lk_padded_dim(1025) == 0
    # above 256: multiples of 64 up to 1024 (csrc/als_big.hip)
    assert [lib.lk_padded_dim(k) for k in (257, 320, 321, 512, 1000, 1024)] == [
        320, 320, 384, 512, 1024, 1024]
    # argument validation happens before any device work
    h = ctypes.c_void_p(0)
    rc = lib.lk_als_plan_create(ctypes.byref(h), None, 0, 10, 64, 0)
    assert rc == _native.LK_E_INVALID and b"null" in lib.lk_last_error()
    assert lib.lk_gramian_workspace_bytes(64) > 0 and lib.lk_gramian_workspace_bytes(1300) == 0
    assert lib.lk_gramian_workspace_bytes(300) > 0


def test_no_cpu_fallback():
    """The product path must fail loudly without a GPU -- never route to the oracle."""
    import torch

    from lkpy_amd import _native

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_native.BackendUnavailable):
        _native.require_gpu()
    from lkpy_amd import _device

    with pytest.raises(_native.BackendUnavailable):
        _device.device("cuda")


def test_product_package_never_imports_the_oracle():
    import pathlib
    import re

    pkg = pathlib.Path(__file__).resolve().parent.parent / "lkpy_amd"
    for f in pkg.rglob("*.py"):
        text = f.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f


def test_integration_doc_names_every_entry_point():
    "INTEGRATION.md is the maintainer's map of the C ABI: nothing exported may be missing from it"
    from pathlib import Path

    from lkpy_amd import _native

    text = (Path(__file__).resolve().parent.parent / "INTEGRATION.md").read_text()
    missing = [s for s in _native.declared_symbols() if s not in text]
    assert not missing, missing


# ---- the binding is derived from include/lkamd.h (lkpy_amd/_native.py::parse_header) ----

_P, _I, _I32, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64
_F, _D, _U32, _U64 = ctypes.c_float, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint64

# one function per rule of the parser, read off the header by hand
_PINNED = {
    "lk_last_error": (ctypes.c_char_p, []),  # char * result, (void)
    "lk_task_ctl_destroy": (None, [_P]),  # void result
    "lk_task_ctl_create": (_I, [_P]),  # T **out
    "lk_gramian_workspace_bytes": (ctypes.c_size_t, [_I32]),
    "lk_funksvd_lds_column_bytes": (ctypes.c_size_t, []),
    "lk_gramian": (_I, [_P, _I64, _I32, _I32, _F, _P, _I32, _P, _P]),
    "lk_bias_fit_pass": (_I, [_P, _I, _P, _P, _I64, _D, _P, _I64, _D, _P, _P]),
    "lk_synth_zipf_rows": (_I, [_P, _I64, _I64, _U64, _P, _I64, _P, _P]),
    "lk_stochastic_keys": (_I, [_P, _I64, _I64, _I64, _P, _P, _I32, _F, _P, _U64, _P, _U32, _P,
                                _I64, _P]),
    "lk_flexmf_step": (_I, [_P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P]),  # struct pointers
    "lk_adamw_dense": (_I, [_P, _P, _P, _P, _I64, _I32, _I32] + [_D] * 7 + [_P]),
    "lk_iknn_recommend": (_I, [_P, _P, _P, _I64, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I, _P,
                               _I64, _P, _P, _P, _P]),  # 19 parameters over seven lines
}  # fmt: skip


@pytest.mark.parametrize("name", sorted(_PINNED))
def test_derived_signature(name):
    from lkpy_amd import _native

    lib = _native.load(build_if_missing=True)
    res, args = _PINNED[name]
    assert _native.PROTOTYPES[name] == (res, args)
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args


def test_every_declared_function_is_typed_from_its_prototype():
    import re

    from lkpy_amd import _native

    lib = _native.load(build_if_missing=True)
    names = _native.declared_symbols()
    assert len(names) >= 175 and names == sorted(_native._declare(lib))
    text = re.sub(r"/\*.*?\*/", "", _native.HEADER_PATH.read_text(), flags=re.S)
    for name in names:
        fn = getattr(lib, name)
        res, args = _native.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args, name
        # the number of parameters, counted without the parser: the commas of the declaration
        (params,) = re.findall(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        count = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(fn.argtypes) == count, name


@pytest.mark.parametrize("text, why", [
    ("int lk_f(long n);", "unknown type 'long'"),
    ("unsigned lk_f(void);", "unknown type 'unsigned'"),
    ("int lk_f(int32_t n, float w[4]);", "array"),
    ("int lk_f(void *d, int (*done)(int));", "function pointer"),
    ("int lk_f(const char *fmt, ...);", "variable arguments"),
    # what the symbol pattern finds and the prototype pattern does not must not vanish
    ("int lk_f(int n);\nint lk_g(int n) { return n; }", r"not a prototype.*\['lk_g'\]"),
    ("int lk_f(int n);\nint lk_g(int n) LK_API;", r"not a prototype.*\['lk_g'\]"),
], ids=["type", "result", "array", "function-pointer", "varargs", "definition", "attribute"])
def test_parser_refuses_what_it_does_not_know(text, why):
    from lkpy_amd import _native

    with pytest.raises(ValueError, match="lkamd.h: .*" + why):
        _native.parse_header(text)


def test_parser_reads_a_small_header():
    from lkpy_amd import _native

    protos, defines = _native.parse_header(
        "#define LK_A 3 /* three */\n#define LK_B (-2)\n#define LK_S \"s\"\n#define OTHER 1\n"
        "#if 0\nint lk_later(long x);\n#endif /* planned */\n"
        "typedef struct lk_h lk_h;\n/* lk_gone(int) */\n"
        "const char *lk_name(void);\nconst float *lk_at(const lk_h *h,\n   int64_t i);\n"
        "void lk_free(lk_h **h);\n")
    assert defines == {"LK_A": 3, "LK_B": -2}
    assert protos == {"lk_name": (ctypes.c_char_p, []), "lk_at": (_P, [_P, _I64]),
                      "lk_free": (None, [_P])}


def test_every_integer_define_is_parsed_and_the_constants_are_the_headers():
    import re

    from lkpy_amd import _native

    text = _native.HEADER_PATH.read_text()
    found = {m[0]: int(m[1]) for m in re.findall(r"#define (LK_\w+) \(?(-?\d+)\)?", text)}
    assert len(found) >= 38 and found == _native.H
    assert (_native.LK_OK, _native.LK_E_INVALID, _native.LK_E_CANCELLED) == (0, -1, -6)
    assert _native.SOLVER_AUTO == found["LK_SOLVER_AUTO"] == 2
    assert _native.GEMM_K_FROM_ROW == found["LK_GEMM_K_FROM_ROW"] == 4
    assert _native.STOCHASTIC_TRANSFORMS == {None: 0, "softmax": 1, "linear": 2}
    assert _native.SPARSE_REDUCTIONS == {"sum": 0, "mean": 1, "max": 2}
    assert (_native.BMF_INVALID, _native.BMF_FOLD, _native.BMF_STORED) == (0, 1, 2)
    assert (found["LK_ALS_PLAN_REFERENCE_ORDER"], found["LK_ALS_PLAN_HYBRID_ORDER"],
            found["LK_ALS_PLAN_BAND_UNITS"]) == (1, 2, 4)


@pytest.mark.parametrize("struct, cls, size", [
    ("lk_flexmf_tables", "FlexMFTables", 120),  # 12 pointers, 2 int64_t, 1 int32_t + padding
    ("lk_flexmf_hyper", "FlexMFHyper", 80),  # 4 int32_t, 8 doubles
])
def test_flexmf_structs_follow_the_header(struct, cls, size):
    import re

    from lkpy_amd import _native

    text = re.sub(r"/\*.*?\*/", "", _native.HEADER_PATH.read_text(), flags=re.S)
    (body,) = re.findall(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S)
    fields = []
    for decl in body.split(";"):
        # `int64_t n_users, n_items` / `float *param[4]`: the names after the type
        names = re.sub(r"\[\d+\]", "", decl).replace("*", " ").split()[1:]
        fields += [n.rstrip(",") for n in names]
    cls = getattr(_native, cls)
    assert fields and fields == [f[0] for f in cls._fields_]
    assert ctypes.sizeof(cls) == size
