"""CPU: the C-ABI library loads without a GPU and exports every function include/gple.h declares."""
import ctypes
import os
import re

from gaussian_process_liouville_equation_amd import _capi
from tests.conftest import ROOT


def declared_functions():
    text = open(os.path.join(ROOT, "include", "gple.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gple_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_agree():
    names = declared_functions()
    assert len(names) >= 20
    assert sorted("gple_" + n for n in _capi.GPLE_SYMBOLS) == names


def header_prototypes():
    """{name: (result type, [argument declarations])} of every function include/gple.h declares"""
    text = open(os.path.join(ROOT, "include", "gple.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.findall(r"^[ \t]*((?:const\s+)?\w+(?:\s+\w+)*\s*\**)\s*\b(gple_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M)
    enums = set(re.findall(r"typedef\s+enum\s+(\w+)", text))
    return {name: (" ".join(res.split()), [" ".join(a.split()) for a in args.split(",")]) for res, name, args in found}, enums


INTEGER_TYPES = {"int", "unsigned", "long", "size_t", "unsigned long long", "unsigned char"}


def c_class(declaration, enums):
    """pointer / integer / double of one C parameter declaration `type name`; enums and size_t / unsigned long long are integers, every other
    type name that is not double (handles, structs, the callback typedefs) is a pointer"""
    if "*" in declaration or "[" in declaration:
        return "pointer"
    type_name = " ".join(w for w in declaration.split()[:-1] if w != "const")
    return "double" if type_name == "double" else "integer" if type_name in INTEGER_TYPES | enums else "pointer"


def ctypes_class(t):
    if t is ctypes.c_double:
        return "double"
    if t in (ctypes.c_int, ctypes.c_uint, ctypes.c_long, ctypes.c_size_t, ctypes.c_ulonglong):
        return "integer"
    assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)), t
    return "pointer"


def test_declared_signatures_match_the_header():
    """Every function of include/gple.h carries, once the library is loaded, as many argument types as its prototype has parameters, each of
    the prototype's class (pointer / integer / double), and the prototype's result type"""
    import gaussian_process_liouville_equation_amd as pkg

    prototypes, enums = header_prototypes()
    assert sorted(prototypes) == declared_functions()
    lib = pkg.load_library()
    results = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
    for name, (result, params) in prototypes.items():
        f = getattr(lib, name)
        assert f.restype is results[result.replace(" *", "*")], name
        assert f.argtypes is not None and len(f.argtypes) == len(params), (name, f.argtypes, params)
        for k, (t, declaration) in enumerate(zip(f.argtypes, params)):
            assert ctypes_class(t) == c_class(declaration, enums), (name, k, t, declaration)


def test_hip_library_exports_every_declared_symbol():
    import gaussian_process_liouville_equation_amd as pkg

    lib = pkg.load_library()  # no HIP call happens at load time, so this works on a CPU-only machine
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert lib.gple_status_string(0) == b"ok"


def test_oracle_exports_the_mirror_interface():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libgple_oracle.so"))
    for name in ["real_gram", "cutoff_factor", "real_fit_create", "real_fit_release", "real_fit_get", "real_predict",
                 "complex_fit_create", "complex_fit_release", "complex_fit_get", "complex_predict", "loose_function", "nlml",
                 "nlml_predict", "nlml_cross", "nlml_cross_predict", "complex_gram"]:
        assert hasattr(lib, "oracle_" + name), name


def test_product_never_imports_the_oracle():
    pkg_dir = os.path.join(ROOT, "gaussian_process_liouville_equation_amd")
    for base, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                text = open(os.path.join(base, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "libgple_oracle" not in text and "gple_oracle.h" not in text, os.path.join(base, f)
