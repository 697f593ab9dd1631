"""CPU-only: fgnn_hip/lib.py types the kernel library from ONE table, and that table and the ctypes structures are what
include/fgnn_hip.h declares -- every prototype translated by rule, every structure laid out as the C compiler lays it."""
import ctypes as C
import os
import re
import subprocess

from test_capi_exports import ROOT, _declared

HEADER = os.path.join(ROOT, "include", "fgnn_hip.h")
SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double}


def _header():
    """the header without comments and preprocessor lines"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", txt, flags=re.M)


def _scalar(ctype, where):
    ctype = re.sub(r"^const ", "", ctype)
    assert ctype in SCALARS, "no rule for the type %r of %s" % (ctype, where)
    return SCALARS[ctype]


def _prototypes():
    """{name: (restype, argtypes)} of every function the header declares: a pointer or array is a c_void_p (a returned
    const char * a c_char_p), void returns None, a scalar is its ctypes twin"""
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\n]*?[\s*]+)(fgnn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()):
        ret, params = " ".join(ret.split()), " ".join(params.split())
        if "*" in ret:
            restype = C.c_char_p if ret.replace(" ", "") == "constchar*" else C.c_void_p
        else:
            restype = None if ret == "void" else _scalar(ret, name)
        argtypes = []
        for p in [] if params == "void" else params.split(","):
            p = p.strip()
            if "*" in p or p.endswith("]"):
                argtypes.append(C.c_void_p)
            else:
                ctype, _, pname = p.rpartition(" ")
                argtypes.append(_scalar(ctype, "%s(%s)" % (name, pname)))
        assert name not in out, name
        out[name] = (restype, tuple(argtypes))
    return out


def test_signature_table_equals_the_header():
    from fgnn_hip import lib
    protos = _prototypes()
    # a prototype the parser cannot read is a failure, not a gap: it finds what the export test's name search finds
    assert sorted(protos) == _declared("fgnn_hip.h")
    assert sorted(lib.SIGNATURES) == sorted(protos)
    for name, sig in protos.items():
        assert lib.SIGNATURES[name] == sig, name
    assert lib.EXPORTS == list(lib.SIGNATURES)


def test_every_function_of_the_loaded_library_is_typed():
    from fgnn_hip import lib
    L = lib.load()
    for name, (restype, argtypes) in lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name


STRUCTS = {"fgnn_debug_scan_state": "DebugScanState", "fgnn_copy_segment": "CopySegment", "fgnn_extract_job": "ExtractJob",
           "fgnn_sampler_config": "SamplerConfig", "fgnn_batch_meta": "BatchMeta", "fgnn_run_plan": "RunPlan"}


def _struct_fields(cname):
    """field names of `typedef struct [tag] { ... } cname;`, in order"""
    body = re.search(r"typedef struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*%s\s*;" % cname, _header())
    assert body, cname
    names = []
    for decl in body.group(1).split(";"):
        if decl.strip():
            for d in decl.split(","):
                names.append(re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", d).group(1))
    return names


def test_structures_match_the_headers_layout(tmp_path):
    from fgnn_hip import lib
    fields = {c: _struct_fields(c) for c in STRUCTS}
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "fgnn_hip.h"', "int main(void) {"]
    for c, names in fields.items():
        src.append('  printf("%s %%zu\\n", sizeof(%s));' % (c, c))
        src += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c, f, c, f) for f in names]
    src += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "layout.c")])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    for c, pyname in STRUCTS.items():
        cls = getattr(lib, pyname)
        assert [f[0] for f in cls._fields_] == fields[c], c
        assert C.sizeof(cls) == int(got[c]), c
        for f in fields[c]:
            assert getattr(cls, f).offset == int(got["%s.%s" % (c, f)]), (c, f)
