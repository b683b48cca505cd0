"""CPU-only: the C-ABI library loads and exports every symbol include/bcx.h declares, the binding's signatures, constants and
structs are the header's (bayesiancoresets_amd/_abi.py parses it), and the parser refuses what it cannot read; the product path
fails loudly (no CPU fallback) when no GPU is usable."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "bcx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bcx_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_exported():
    from bayesiancoresets_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _native.load()
    declared = _declared_symbols()
    assert len(declared) >= 126
    for name in declared:
        assert hasattr(lib, name), "libbcx.so does not export " + name
    assert len(_native.SYMBOLS) == len(declared), "the header parser and this test's regex count different prototypes"
    assert sorted(_native.SYMBOLS) == declared, "python binding list out of sync with include/bcx.h"
    assert lib.bcx_version().decode().startswith("bcx ")


def test_signatures_spelled_by_hand():
    """What load() set from the header against signatures written out here by hand, one for every form of the grammar: struct
    pointer and pointer to pointer, const void**, uint64_t, float*, a struct array among 24 parameters, 33 parameters, a double
    between integers, (void) with a const char* return, an int32_t return, int64_t returns."""
    from bayesiancoresets_amd import _native
    lib = _native.load()
    vp, i32, i64, u64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    spelled = {
        "bcx_create": (ctypes.c_int, [vp, vp]),
        "bcx_load_rows_flags": (ctypes.c_int, [vp, vp, i32, i32, i64, i64, i64, i32]),
        "bcx_chunk_sums": (ctypes.c_int, [vp, vp, vp, vp]),
        "bcx_standard_normal": (ctypes.c_int, [vp, u64, u64, i64, vp]),
        "bcx_screen_read": (ctypes.c_int, [vp, i64, i64, vp, vp, vp, vp]),
        "bcx_nuts_batch": (ctypes.c_int, [vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, dbl, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp,
                                          i32, vp, vp]),
        "bcx_cmc_advance": (ctypes.c_int, [vp, i32, i32, i32, vp, vp, i64, vp, vp, i64, i32, i32, i32, dbl, i32, i32, i32, vp, vp, vp,
                                           i64, i64, vp, i64, vp, i64, vp, i32, vp, vp, vp, vp, vp]),
        "bcx_build_begin": (ctypes.c_int, [vp, i64, dbl, vp]),
        "bcx_exchange_attach": (ctypes.c_int, [vp, vp, i32, dbl]),
        "bcx_project_last_error": (ctypes.c_char_p, []),
        "bcx_version": (ctypes.c_char_p, []),
        "bcx_last_error": (ctypes.c_char_p, [vp]),
        "bcx_nuts_adapt_schedule": (ctypes.c_int32, [i32, vp, i32]),
        "bcx_project_select_scratch_bytes": (ctypes.c_int64, [i32, i64, i32]),
        "bcx_log_predictive_scratch_bytes": (ctypes.c_int64, [i64, i32, i64, i32]),
    }
    assert len(spelled["bcx_nuts_batch"][1]) == 24 and len(spelled["bcx_cmc_advance"][1]) == 33
    for name, (restype, argtypes) in spelled.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name
    for name in _native.SYMBOLS:        # nothing the header declares is left with ctypes' defaults
        assert getattr(lib, name).argtypes is not None, name


_GOOD = """
/* a comment with bcx_not_a_call( in it */
#ifndef X_H
#define BCX_LIMIT 12
enum { BCX_A = 0, BCX_B = -3 };   // BCX_C = 7
typedef struct bcx_rec { const void* p; int64_t n; int32_t k; } bcx_rec;
typedef struct bcx_handle bcx_handle;
int bcx_one(bcx_handle* h, const bcx_rec* recs, const void** out, double x,
            uint64_t seed);
int64_t bcx_two(void);
const char* bcx_three(const bcx_handle* h);
#endif
"""


def test_parser_reads_the_grammar():
    from bayesiancoresets_amd import _abi
    vp = ctypes.c_void_p
    consts, structs, protos = _abi.parse(_GOOD)
    assert consts == {"BCX_LIMIT": 12, "BCX_A": 0, "BCX_B": -3}
    assert list(structs) == ["bcx_rec"] and structs["bcx_rec"]._fields_ == [("p", vp), ("n", ctypes.c_int64), ("k", ctypes.c_int32)]
    assert protos == {"bcx_one": (ctypes.c_int, [vp, vp, vp, ctypes.c_double, ctypes.c_uint64]), "bcx_two": (ctypes.c_int64, []),
                      "bcx_three": (ctypes.c_char_p, [vp])}


@pytest.mark.parametrize("decl, named", [
    ("int bcx_bad(void* s, float x);", "bcx_bad"),                     # a scalar type outside the table
    ("int bcx_bad(void* s, int n);", "bcx_bad"),                       # plain int is a return type only
    ("int bcx_bad(void* s, int32_t);", "bcx_bad"),                     # a parameter without a name
    ("int bcx_bad(void* s, const void*);", "bcx_bad"),
    ("int bcx_bad(bcx_rec r);", "bcx_bad"),                            # a struct by value
    ("int bcx_bad(void* s, int32_t v[4]);", "bcx_bad"),                # an array declarator
    ("int bcx_bad(void* s, void (*cb)(int32_t a));", "bcx_bad"),       # a function pointer
    ("float bcx_bad(void* s);", "bcx_bad"),                            # a return type outside the table
    ("int bcx_bad(void* s, int32_t n;", "bcx_bad"),                    # an unmatched parenthesis: nothing is skipped
    ("int bcx_bad void* s);", "bcx_bad"),
    ("int bcx_two(void);", "occurs 4 times"),                           # declared twice: the count of `bcx_name(` disagrees
    ("enum { BCX_D };", "BCX_D"),                                      # an enum entry without an explicit value
    ("typedef struct bcx_s { float f; } bcx_s;", "bcx_s"),             # a field type outside the table
])
def test_parser_refuses_what_it_cannot_read(decl, named):
    from bayesiancoresets_amd import _abi
    with pytest.raises(ValueError) as e:
        _abi.parse(_GOOD.replace("int64_t bcx_two(void);", "int64_t bcx_two(void);\n" + decl))
    assert named in str(e.value)
    _abi.parse(_GOOD)


def test_missing_header_is_an_error(tmp_path):
    """No header, no binding: the error names where it was looked for (a source checkout's include/, an installed package's _lib/)."""
    from bayesiancoresets_amd import _abi
    assert _abi.header_path() == os.path.join(ROOT, "include", "bcx.h")
    here = str(tmp_path / "top" / "package")
    with pytest.raises(RuntimeError) as e:
        _abi.header_path(here)
    assert os.path.join(str(tmp_path), "include", "bcx.h") in str(e.value) and os.path.join(here, "_lib", "bcx.h") in str(e.value)
    os.makedirs(os.path.join(here, "_lib"))
    open(os.path.join(here, "_lib", "bcx.h"), "w").close()
    assert _abi.header_path(here) == os.path.join(here, "_lib", "bcx.h")


def test_config_struct_layout():
    """ctypes mirror of bcx_config matches the C layout (8 int32 then 3 int64 = 56 bytes)."""
    import ctypes
    from bayesiancoresets_amd import _native
    assert ctypes.sizeof(_native.Config) == 56
    assert _native.Config.n_local.offset == 32


def test_nuts_problem_struct_layout():
    """bcx_nuts_problem: two pointers, an int64, two pointers, an int64, two int32 = 56 bytes."""
    from bayesiancoresets_amd import _native
    assert ctypes.sizeof(_native.NutsProblem) == 56
    assert _native.NutsProblem.k.offset == 48
    assert [n for n, _ in _native.NutsProblem._fields_] == ["w_dev", "pts_dev", "ldp", "mu_dev", "W_dev", "ldw", "k", "index"]


def test_codes_as_numbered_today():
    """The return codes and the per-iteration states, written out: a renumbering in the header has to be made here too."""
    from bayesiancoresets_amd import _native as n
    assert (n.OK, n.ERR_ARG, n.ERR_HIP, n.ERR_ZERO_ROW, n.ERR_ZERO_B, n.ERR_NOMEM, n.ERR_STATE, n.ERR_EXCHANGE, n.ERR_TIMEOUT) == \
        (0, -1, -2, -3, -4, -5, -6, -7, -8)
    assert (n.IT_OK, n.IT_FAIL_SELECT, n.IT_FAIL_REWEIGHT, n.IT_FAIL_MONOTONE) == (0, 1, 2, 3)
    assert (n.ALG_GIGA, n.ALG_FW, n.ALG_OMP) == (0, 1, 2) and (n.F32, n.F64, n.F16) == (0, 1, 2)
    assert n.Engine.SCREEN4_MAX_WAVES == n.SCREEN4_MAX_WAVES == 2048


def test_row_length_limit_matches_header():
    from bayesiancoresets_amd import _native
    text = open(os.path.join(ROOT, "include", "bcx.h")).read()
    assert int(re.search(r"#define\s+BCX_MAX_ROW_LENGTH\s+(\d+)", text).group(1)) == _native.MAX_ROW_LENGTH
    assert int(re.search(r"#define\s+BCX_LOAD_CENTER_ROWS\s+(\d+)", text).group(1)) == _native.LOAD_CENTER_ROWS


def test_no_cpu_fallback():
    """Without a GPU the solver constructors raise; they never fall back to host arithmetic."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import bayesiancoresets_amd as bc
    from bayesiancoresets_amd import _native
    X = np.random.RandomState(0).randn(32, 4)
    for cls in (bc.snnls.GIGA, bc.snnls.FrankWolfe, bc.snnls.OrthoPursuit):
        with pytest.raises(_native.EngineError):
            cls(X.T, X.sum(axis=0))


def test_product_does_not_import_oracle():
    """oracle/ is test infrastructure: nothing under bayesian-coresets_amd/ may import or load it."""
    pkg = os.path.join(ROOT, "bayesian-coresets_amd")
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|snnls_oracle|oracle/_ref", re.M)
    for dp, dn, fn in os.walk(pkg):
        for f in fn:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f), errors="ignore").read()
                assert not pat.search(src), os.path.join(dp, f)
