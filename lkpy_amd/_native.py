"""
ctypes binding of the C ABI declared in ``include/lkamd.h`` (``lkpy_amd/_lkamd.so``).

The header is the only description of the ABI: :func:`parse_header` reads every ``lk_*``
prototype and every integer ``#define LK_*`` from it when this module is imported, and
:func:`load` sets each function's ``restype`` / ``argtypes`` from that.  A new entry point
needs its prototype in the header, its wrapper in ``_device.py`` and its mention in
``INTEGRATION.md``, nothing here; a new constant needs its ``#define`` and, if Python names
it, one line below.  Only the two ``lk_flexmf_*`` structs are written out again
(tests/test_native_abi.py pins them to the header).

The product path has NO CPU fallback: if the HIP library is missing or there is no
GPU, the calls raise (:class:`BackendUnavailable`).  Loading the library and listing
its symbols works without a GPU (used by the CPU-only tests).
"""

from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_int32, c_int64, c_void_p
from pathlib import Path

_PKG = Path(__file__).resolve().parent
# LK_AMD_LIBRARY: load another build of the library (kernel-variant experiments)
LIB_PATH = Path(os.environ.get("LK_AMD_LIBRARY", _PKG / "_lkamd.so"))
HEADER_PATH = _PKG.parent / "include" / "lkamd.h"

_SCALARS = {"int": ctypes.c_int, "int32_t": c_int32, "int64_t": c_int64,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(LK_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)
_SYMBOL = re.compile(r"\b(lk_[a-z0-9_]+)\s*\(")
# result type, name, parameter list of `<type> lk_name(<parameters>);` at statement level
_PROTOTYPE = re.compile(
    r"(?:\A|(?<=[;{}]))\s*([A-Za-z_][\w\s*]*?)" + _SYMBOL.pattern + r"([^;{}]*)\)\s*;")


def _ctype(decl: str, result: bool = False):
    "The ctypes type of one parameter declaration (or result type); no guess at an unknown one."
    if re.search(r"[\[()]|\.\.\.", decl):
        raise ValueError(f"lkamd.h: array, function pointer or variable arguments in {decl!r}")
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return c_char_p if result and words == ["char", "*"] else c_void_p
    base = " ".join(words if result or len(words) == 1 else words[:-1])  # less the parameter's name
    if result and base == "void":
        return None
    if base not in _SCALARS:
        raise ValueError(f"lkamd.h: unknown type {base!r} in {decl!r}")
    return _SCALARS[base]


def parse_header(text: str):
    """
    ``(prototypes, defines)`` of a header text: ``{name: (restype, argtypes)}`` of every ``lk_*``
    function and ``{LK_NAME: int}`` of every integer ``#define``.  Every pointer is a
    ``c_void_p`` (handles, ``T **out``, device and host arrays, the structs), but a ``char *``
    result is a ``c_char_p``.  Raises ``ValueError`` on anything outside that.
    """
    text = re.sub(r"#if 0.*?#endif /\* planned \*/", "", text, flags=re.S)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    defines = {name: int(value) for name, value in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    prototypes = {}
    for res, name, params in _PROTOTYPE.findall(text):
        params = params.strip()
        args = [] if params in ("", "void") else [_ctype(p) for p in params.split(",")]
        prototypes[name] = (_ctype(res, result=True), args)
    skipped = set(_SYMBOL.findall(text)) - set(prototypes)
    if skipped:
        raise ValueError(f"lkamd.h: not a prototype this binding can read: {sorted(skipped)}")
    return prototypes, defines


PROTOTYPES, H = parse_header(HEADER_PATH.read_text())

LK_OK = H["LK_OK"]
LK_E_INVALID = H["LK_E_INVALID"]
LK_E_HIP = H["LK_E_HIP"]
LK_E_NOT_SPD = H["LK_E_NOT_SPD"]
LK_E_NAN_SIM = H["LK_E_NAN_SIM"]
LK_E_NOMEM = H["LK_E_NOMEM"]
LK_E_CANCELLED = H["LK_E_CANCELLED"]

SOLVER_CHOLESKY = H["LK_SOLVER_CHOLESKY"]
SOLVER_CG = H["LK_SOLVER_CG"]
SOLVER_AUTO = H["LK_SOLVER_AUTO"]

FLEXMF_LOSSES = {"logistic": H["LK_FLEXMF_LOGISTIC"], "pairwise": H["LK_FLEXMF_PAIRWISE"],
                 "warp": H["LK_FLEXMF_WARP"]}
FLEXMF_MSE = H["LK_FLEXMF_MSE"]  # lk_flexmf_step_explicit's loss
FLEXMF_ADAMW = H["LK_FLEXMF_ADAMW"]
FLEXMF_SPARSE_ADAM = H["LK_FLEXMF_SPARSE_ADAM"]
FLEXMF_MAX_K = H["LK_FLEXMF_MAX_K"]

STOCHASTIC_TRANSFORMS = {None: H["LK_STOCHASTIC_NONE"], "softmax": H["LK_STOCHASTIC_SOFTMAX"],
                         "linear": H["LK_STOCHASTIC_LINEAR"]}

FAIR_MAX_N = H["LK_FAIR_MAX_N"]  # (lk_fair_max_n()): the list length lk_fair_rerank's LDS holds

# a query's branch of BiasedMFScorer.__call__
BMF_INVALID, BMF_FOLD, BMF_STORED = H["LK_BMF_INVALID"], H["LK_BMF_FOLD"], H["LK_BMF_STORED"]

ASSOC_METHODS = {"probability": H["LK_ASSOC_PROBABILITY"], "lift": H["LK_ASSOC_LIFT"]}
ASSOC_REDUCTIONS = {"mean": H["LK_ASSOC_MEAN"], "max": H["LK_ASSOC_MAX"]}
SPARSE_REDUCTIONS = {"sum": H["LK_SPARSE_SUM"], "mean": H["LK_SPARSE_MEAN"],
                     "max": H["LK_SPARSE_MAX"]}
# lk_gemm_f32's tile mask
GEMM_LOWER = H["LK_GEMM_LOWER"]
GEMM_K_FROM_COL = H["LK_GEMM_K_FROM_COL"]
GEMM_K_FROM_ROW = H["LK_GEMM_K_FROM_ROW"]
FUNKSVD_GLOBAL_COLUMNS = H["LK_FUNKSVD_GLOBAL_COLUMNS"]  # lk_funksvd_train_feature's flag


class FlexMFTables(ctypes.Structure):
    "``lk_flexmf_tables``: u_embed, i_embed, u_bias, i_bias and their two moment tables."
    _fields_ = [("param", c_void_p * 4), ("exp_avg", c_void_p * 4), ("exp_avg_sq", c_void_p * 4),
                ("n_users", c_int64), ("n_items", c_int64), ("k", c_int32)]


class FlexMFHyper(ctypes.Structure):
    "``lk_flexmf_hyper``"
    _fields_ = [("loss", c_int32), ("optimizer", c_int32), ("l2", c_int32), ("n_neg", c_int32),
                ("pos_weight", ctypes.c_double), ("reg", ctypes.c_double),
                ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("bias_corr1", ctypes.c_double),
                ("bias_corr2", ctypes.c_double)]


class BackendUnavailable(RuntimeError):
    "The HIP extension or the GPU is missing; there is deliberately no CPU fallback."


_lib = None


def _declare(lib):
    "Give every function of the header its types on ``lib``; returns name -> (restype, argtypes)."
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return PROTOTYPES


def load(build_if_missing: bool = False):
    "Load ``_lkamd.so``; raises :class:`BackendUnavailable` if it is not built."
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        if build_if_missing:
            from .csrc.build import build

            build()
        else:
            raise BackendUnavailable(
                f"{LIB_PATH} not found: build it with `python -m lkpy_amd.csrc.build` "
                "(or __graft_entry__.build()); lkpy_amd has no CPU fallback"
            )
    # ONE HIP runtime per process: the PyTorch-ROCm wheel bundles its own libamdhip64 /
    # libhsa-runtime64, and whichever copy is mapped first serves everybody (same sonames).  If
    # this library came first it would pull /opt/rocm's copy and torch's bundled HSA runtime would
    # then find no device ("No HIP GPUs are available": seen when __graft_entry__.build() loaded
    # the library before smoke() imported torch).  torch is the device-memory plumbing of this
    # package anyway, so it is imported here, before the dlopen.
    import torch  # noqa: F401

    try:
        lib = ctypes.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover
        raise BackendUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    _declare(lib)
    _lib = lib
    return lib


def declared_symbols() -> list[str]:
    "Every function ``include/lkamd.h`` declares (used by the export test)."
    return sorted(PROTOTYPES)


def last_error() -> str:
    return load().lk_last_error().decode()


def check(rc: int, what: str = "lkamd call"):
    "Map a C-ABI return code to the exception the reference raises for it."
    if rc == LK_OK:
        return
    msg = last_error()
    if rc == LK_E_NOT_SPD:
        # src/accel/als/implicit.rs:79 -> RuntimeError("ALS solve error: ...")
        raise RuntimeError(msg)
    if rc == LK_E_NAN_SIM:
        raise ValueError("similarity is null")  # src/accel/knn/accum.rs:146-151
    if rc == LK_E_INVALID:
        raise ValueError(f"{what}: {msg}")
    if rc == LK_E_CANCELLED:
        raise KeyboardInterrupt(msg)
    raise RuntimeError(f"{what} failed ({rc}): {msg}")


def require_gpu():
    "Raise unless the library is loaded and a HIP device is visible."
    lib = load()
    if lib.lk_device_count() < 1:
        raise BackendUnavailable("no HIP device visible; lkpy_amd has no CPU fallback")
    return lib
