"""The ctypes binding is derived from include/mimi_hip.h (mimi_amd/_header.py reads it, mimi_amd/_capi.py builds on it).
(1) the reader on literal snippets: every construct of the header's subset is accepted, everything else is refused with the
offending text; (2) the struct layouts, enumerators and defines it reads against the host C compiler on the same header;
(3) after lib() every declared function carries argtypes and restype, counted independently here; (4) importing the
front-ends parses the header and loads no library; (5) an edited prototype changes the derived argtypes."""
import ctypes as C
import keyword
import os
import re
import shutil
import subprocess
import sys

import pytest

from mimi_amd import _capi, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mimi_hip.h")
STRUCTS = {"mimi_hip_material": _capi.Material, "mimi_hip_domain_tables": _capi.DomainTables,
           "mimi_hip_bspline_patch": _capi.BSplinePatch, "mimi_hip_contact_tables": _capi.ContactTables,
           "mimi_hip_pressure_tables": _capi.PressureTables, "mimi_hip_spline_body": _capi.SplineBody}


def header_text():
    with open(HEADER) as f:
        return f.read()


# ---- (1) the reader on literal snippets ----------------------------------------------------------------------------------

def test_comments_preprocessor_lines_and_the_extern_c_wrapper_are_dropped():
    h = _header.parse('/* int gone(int x); */\n#ifndef X_H\n#define X_H\n#include <stdint.h>\n#ifdef __cplusplus\n'
                      'extern "C" {\n#endif\nint kept(int /* what */ x);\n#ifdef __cplusplus\n}\n#endif\n#endif /* X_H */\n')
    assert h.functions == {"kept": (C.c_int, [C.c_int])} and not h.structs and not h.enums and not h.defines


def test_integer_defines_are_kept_and_other_defines_ignored():
    h = _header.parse("#define MIMI_HIP_H\n#define VERSION 12\n#define MASK 0x10\n#define NEG -3\n"
                      "#define STREAM_NULL ((void*)(intptr_t)-1)\n#define TWICE(x) 2 * x\n")
    assert h.defines == {"VERSION": 12, "MASK": 16, "NEG": -3}


def test_enum_with_explicit_values():
    h = _header.parse("enum kind {\n  A = 0, /* first */\n  B = 1,\n  C = 5\n};\nenum other { D = -1 };")
    assert h.enums == {"A": 0, "B": 1, "C": 5, "D": -1}


def test_opaque_handle_by_value_and_by_pointer():
    h = _header.parse("typedef struct x_s* x_t;\nint f(x_t h, x_t* out);")
    assert h.functions["f"] == (C.c_int, [C.c_void_p, C.c_void_p])


def test_struct_fields_scalars_pointers_arrays_and_several_declarators():
    h = _header.parse("typedef struct s {\n  int32_t kind; /* k */\n  int64_t n;\n  double density, lambda, mu;\n"
                      "  const double* x;\n  int32_t degree[3];\n  const double* knots[3];\n  double body[8], more[2];\n"
                      "  unsigned char flag;\n  size_t bytes;\n  int plain;\n} s;")
    assert h.structs == {"s": [("kind", C.c_int32), ("n", C.c_int64), ("density", C.c_double), ("lambda_", C.c_double),
                               ("mu", C.c_double), ("x", C.c_void_p), ("degree", C.c_int32 * 3), ("knots", C.c_void_p * 3),
                               ("body", C.c_double * 8), ("more", C.c_double * 2), ("flag", C.c_ubyte),
                               ("bytes", C.c_size_t), ("plain", C.c_int)]}


def test_keyword_field_names_get_a_trailing_underscore():
    fields = _header.parse("typedef struct s { double lambda; int32_t pass, class; double lambda_x; } s;").structs["s"]
    assert [n for n, _ in fields] == ["lambda_", "pass_", "class_", "lambda_x"]


def test_prototypes_scalars_pointers_arrays_void_and_returns():
    h = _header.parse("typedef struct t { int a; } t;\ntypedef struct h_s* h_t;\n"
                      "const char* last_error(void);\nint count(void);\nvoid set(t* m, double young, double poisson);\n"
                      "int64_t info(h_t h, int what);\n"
                      "int sparsity(int32_t dim, const int32_t n_nodes_dir[3], int device, int64_t* rowptr, int64_t n);\n"
                      "int state(h_t h, double* xi, unsigned char* c, size_t bytes, void* stream, const t* tables);")
    assert h.functions == {
        "last_error": (C.c_char_p, []), "count": (C.c_int, []), "set": (None, [C.c_void_p, C.c_double, C.c_double]),
        "info": (C.c_int64, [C.c_void_p, C.c_int]),
        "sparsity": (C.c_int, [C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
        "state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p])}


def test_prototype_broken_over_three_lines():
    h = _header.parse("int gmres(const double* A_values, const double* b, double* x, double rel_tol,\n"
                      "          double abs_tol, int max_iter, int kdim, int preconditioner, int32_t* iterations,\n"
                      "          double* final_norm, int32_t* converged);")
    assert h.functions["gmres"] == (C.c_int, [C.c_void_p] * 3 + [C.c_double] * 2 + [C.c_int] * 3 + [C.c_void_p] * 3)


@pytest.mark.parametrize("text, offending", [
    ("int f(long n);", "long n"),                                                    # an unknown scalar type
    ("typedef struct s { float x; } s;", "float x"),
    ("unsigned f(void);", "unsigned"),
    ("int f(other_t h);", "other_t h"),                                              # a handle nobody declared
    ("int f(struct_nobody_declared* p);", "struct_nobody_declared* p"),
    ("int f(void (*callback)(int), int n);", "void (*callback)(int)"),               # a function-pointer parameter
    ("typedef struct s { int (*callback)(int); } s;", "int (*callback)(int)"),
    ("enum e { A = 0, B };", "B"),                                                   # an enumerator without a value
    ("enum e { A };", "A"),
    ("typedef struct s { int32_t flag : 1; } s;", "int32_t flag : 1"),               # a bit-field
    ("typedef struct s { struct { int a; } inner; } s;", "struct { int a; } inner"),  # a struct nested in a struct
    ("typedef struct t { int a; } t;\ntypedef struct s { t inner; } s;", "t inner"),
    ("int f(int);", "int"),                                                          # a parameter without a name
    ("int f(int a) { return a; }", "return a"),                                      # not a declaration at all
    ("int global;", "int global"),
    ("int f(int a);\nint f(int a);", "int f(int a)"),
])
def test_what_the_reader_does_not_know_is_refused_with_its_text(text, offending):
    with pytest.raises(ValueError) as e:
        _header.parse(text)
    assert offending in str(e.value)


# ---- (2) what the reader takes from the header, against the host C compiler ---------------------------------------------

def run_c(tmp_path, name, body):
    """compile `body` (a main() behind #include "mimi_hip.h") with the host C compiler, run it, return the printed integers"""
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    src, exe = tmp_path / (name + ".c"), tmp_path / name
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mimi_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call([cc, "-std=c99", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    return [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]


def test_struct_layouts_match_the_host_compiler(tmp_path):
    h = _header.parse(header_text())
    assert set(h.structs) == set(STRUCTS)
    assert sum(len(f) for f in h.structs.values()) == 82      # (counted by hand in the header: 24 + 10 + 12 + 8 + 16 + 12)
    c_name = lambda f: f[:-1] if keyword.iskeyword(f[:-1]) else f      # (`lambda_` is the header's `lambda`)
    body, want = "", []
    for name, fields in h.structs.items():
        cls = STRUCTS[name]
        assert cls._fields_ == fields
        body += f'  printf("%zu\\n", sizeof({name}));\n'
        want.append(C.sizeof(cls))
        for field, _ in fields:
            body += f'  printf("%zu %zu\\n", offsetof({name}, {c_name(field)}), sizeof((({name}*)0)->{c_name(field)}));\n'
            want += [getattr(cls, field).offset, getattr(cls, field).size]
    assert run_c(tmp_path, "layouts", body) == want


def test_enumerators_and_defines_match_the_host_compiler(tmp_path):
    h = _header.parse(header_text())
    constants = {**h.enums, **h.defines}
    assert len(h.enums) >= 22 and h.defines == {"MIMI_HIP_ABI_VERSION": 12}
    body = "".join(f'  printf("%lld\\n", (long long){name});\n' for name in constants)
    assert run_c(tmp_path, "constants", body) == list(constants.values())
    # the namespace of the binding holds every enumerator, without the prefix
    assert vars(_capi.ABI) == {k[len("MIMI_HIP_"):]: v for k, v in h.enums.items()}
    assert _capi._header_abi_version() == 12


# ---- (3) every declared function carries its prototype ---------------------------------------------------------------------

def counted_prototypes():
    """name -> (return type text, parameter count), by a regexp over the header and a split on commas: no code shared with
    the reader"""
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^([a-z][\w ]*?\*?)\s*\b(mimi_hip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        out[name] = (ret.strip(), 0 if params.strip() == "void" else len(params.split(",")))
    return out


def test_every_export_has_argtypes_and_restype_after_lib():
    L = _capi.lib()
    protos = counted_prototypes()
    assert sorted(protos) == sorted(_capi.EXPORTS) and len(protos) == 125
    assert sorted(n for n, (ret, _) in protos.items() if ret == "int64_t") == [
        "mimi_hip_contact_action_info", "mimi_hip_domain_info", "mimi_hip_explicit_info", "mimi_hip_fold_info",
        "mimi_hip_follower_action_info", "mimi_hip_linear_info", "mimi_hip_surface_n_points"]
    for name in _capi.EXPORTS:
        fn, (ret, n_params) = getattr(L, name), protos[name]
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, name
        want = {"int64_t": C.c_int64, "const char*": C.c_char_p, "void": None, "int": C.c_int}[ret]
        assert fn.restype is want, name
    assert L.mimi_hip_last_error.restype is C.c_char_p and L.mimi_hip_material_set_young_poisson.restype is None
    assert [n for n in _capi.EXPORTS if len(getattr(L, n).argtypes) == 0] == [
        "mimi_hip_last_error", "mimi_hip_abi_version", "mimi_hip_device_count"]


# ---- (4) imports ----------------------------------------------------------------------------------------------------------------

def test_importing_the_front_ends_loads_no_library():
    code = ("import sys; sys.path.insert(0, %r); import mimi_amd.materials, mimi_amd.integrators; "
            "from mimi_amd import _capi; assert _capi._lib is None and len(_capi.EXPORTS) == 125; "
            "mapped = [l for l in open('/proc/self/maps') if 'libmimi_hip' in l]; assert not mapped, mapped" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_material_kinds_are_the_headers_enumerators():
    import mimi_amd
    enums = _header.parse(header_text()).enums
    hardening = mimi_amd.VoceHardening()
    for cls, name in ((mimi_amd.CompressibleOgdenNeoHookean, "MIMI_HIP_MAT_NEOHOOKEAN"), (mimi_amd.J2, "MIMI_HIP_MAT_J2"),
                      (mimi_amd.StVenantKirchhoff, "MIMI_HIP_MAT_STVK"), (mimi_amd.J2Linear, "MIMI_HIP_MAT_J2LINEAR"),
                      (mimi_amd.J2Simo, "MIMI_HIP_MAT_J2SIMO"), (mimi_amd.J2Log, "MIMI_HIP_MAT_J2LOG")):
        m = cls()
        if hasattr(m, "hardening"):
            m.hardening = hardening
            assert m._c_struct().hardening == enums["MIMI_HIP_HARD_VOCE"] == 1
        assert m._c_struct().kind == enums[name]
    assert [enums["MIMI_HIP_MAT_" + n] for n in ("NEOHOOKEAN", "J2", "STVK", "J2LINEAR", "J2SIMO", "J2LOG")] == [0, 1, 2, 3, 4, 5]


# ---- (5) the binding follows the header ---------------------------------------------------------------------------------------

def test_an_edited_prototype_changes_the_derived_argtypes():
    text = header_text()
    old = "int64_t mimi_hip_domain_info(mimi_hip_domain_t h, int what);"
    assert text.count(old) == 1
    before = _header.parse(text).functions
    after = _header.parse(text.replace(old, "int mimi_hip_domain_info(mimi_hip_domain_t h, int64_t what, double scale);")).functions
    assert before["mimi_hip_domain_info"] == (C.c_int64, [C.c_void_p, C.c_int])
    assert after["mimi_hip_domain_info"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_double])
    assert {n: p for n, p in after.items() if n != "mimi_hip_domain_info"} == \
           {n: p for n, p in before.items() if n != "mimi_hip_domain_info"}
