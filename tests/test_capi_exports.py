"""CPU-only: the C-ABI library builds for gfx950, loads, and exports every symbol include/*.h declares."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b((?:fgnn|samgraph)_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def hip_lib():
    path = os.path.join(ROOT, "fgnn-artifacts_amd", "lib", "libfgnn_hip.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fgnn-artifacts_amd", "csrc")])
    return ctypes.CDLL(path)


def test_fgnn_hip_exports(hip_lib):
    names = _declared("fgnn_hip.h")
    assert len(names) >= 16
    missing = [n for n in names if not hasattr(hip_lib, n)]
    assert not missing, missing


def test_binding_lists_every_export():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import lib
    assert sorted(lib.EXPORTS) == _declared("fgnn_hip.h")


SCAN_DEBUG_ENTRY_POINTS = ["fgnn_debug_scan_block_sums", "fgnn_debug_scan_count", "fgnn_debug_scan_set",
                           "fgnn_debug_scan_get", "fgnn_debug_set_stateless_ticket_start_once"]


def test_scan_debug_entry_points_are_declared_exported_bound_and_documented(hip_lib):
    """the hooks tests/test_scan_wrap_gpu.py drives the single-pass scan's counters with: in the header, in the library,
    in the binding's export list with a signature, and named where INTEGRATION.md lists the debug entry points"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import lib
    declared = _declared("fgnn_hip.h")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SCAN_DEBUG_ENTRY_POINTS:
        assert name in declared and hasattr(hip_lib, name) and name in lib.EXPORTS, name
        assert name in lib.SIGNATURES, name
        assert "`%s`" % name in doc, name
    # the read-back structure of the binding mirrors the header's, field for field
    txt = open(os.path.join(ROOT, "include", "fgnn_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} fgnn_debug_scan_state;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"uint32_t (\w+);", body) == [f for f, _ in lib.DebugScanState._fields_]


PARTITION_DEBUG_ENTRY_POINTS = ["fgnn_debug_set_partition_lds_limit", "fgnn_debug_partition_params"]


def test_partition_debug_entry_points_are_declared_exported_bound_and_documented(hip_lib):
    """the hooks tests/test_hashtable_adversarial_gpu.py places its cases with: in the header, in the library, in the
    binding's export list with a signature, and named where INTEGRATION.md lists the debug entry points; the read-only
    one answers without a GPU, with the values tests/golden/partition_params.json records"""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import lib
    declared = _declared("fgnn_hip.h")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in PARTITION_DEBUG_ENTRY_POINTS:
        assert name in declared and hasattr(hip_lib, name) and name in lib.EXPORTS, name
        assert name in lib.SIGNATURES, name
        assert "`%s`" % name in doc, name
    assert "fgnn_hashtable_capacity" in declared and "fgnn_hashtable_capacity" in lib.EXPORTS
    assert callable(getattr(lib.HashTable, "capacity", None))
    out = (ctypes.c_uint32 * 8)(*([0xDEADBEEF] * 8))
    hip_lib.fgnn_debug_partition_params.restype = None
    hip_lib.fgnn_debug_partition_params(out)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "partition_params.json")))
    assert list(golden) == list(lib.PARTITION_PARAMS)
    assert [int(v) for v in out] == [golden[k] for k in lib.PARTITION_PARAMS]


GATHER_DEBUG_ENTRY_POINTS = ["fgnn_debug_gather_plan"]


def test_gather_debug_entry_point_is_declared_exported_bound_and_documented(hip_lib):
    """the planner tests/test_gather_references.py checks the 32-bit tile walk's bound with: in the header, in the
    library, in the binding's export list with a signature and a wrapper, named where INTEGRATION.md lists the debug
    entry points -- and it answers without a GPU"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import lib
    declared = _declared("fgnn_hip.h")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in GATHER_DEBUG_ENTRY_POINTS:
        assert name in declared and hasattr(hip_lib, name) and name in lib.EXPORTS, name
        assert name in lib.SIGNATURES, name
        assert "`%s`" % name in doc, name
    assert callable(getattr(lib, "debug_gather_plan", None))
    fn = hip_lib.fgnn_debug_gather_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t,
                   ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    out = (ctypes.c_uint64 * 8)(*([0xDEADBEEF] * 8))
    # 5000 rows of 512 bytes = 160000 chunks = 157 tiles of 1024: one launch of 157 workgroups
    assert fn(5000, 512, 0, 1, 0xFFFFFFFF, 256, 4, 4, out, 2) == 1
    assert [int(v) for v in out] == [0, 5000, 157, 1024] + [0xDEADBEEF] * 4
    # 2^32 - 1024 rows of one chunk: the walk of 1024 workgroups would wrap; two slices, or a refusal when device-sized
    assert fn(0xFFFFFC00, 16, 0, 1, 0xFFFFFFFF, 256, 4, 4, out, 2) == 2
    assert [int(v) for v in out] == [0, 1 << 31, 1024, 1024, 1 << 31, 0xFFFFFC00 - (1 << 31), 1024, 1024]
    assert fn(0xFFFFFC00, 16, 1, 1, 0xFFFFFFFF, 256, 4, 4, out, 2) == -1


def test_version_and_scratch(hip_lib):
    hip_lib.fgnn_version.restype = ctypes.c_char_p
    assert b"gfx950" in hip_lib.fgnn_version()
    hip_lib.fgnn_scratch_bytes.restype = ctypes.c_size_t
    hip_lib.fgnn_scratch_bytes.argtypes = [ctypes.c_size_t]
    assert hip_lib.fgnn_scratch_bytes(1000) >= 4000


def test_no_cpu_fallback():
    """The product path must fail loudly without a GPU, not compute on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import lib
    t = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(lib.FgnnError):
        lib.sample_khop("khop2", t, t, t, 2, 0, 0, 0)
    with pytest.raises(lib.FgnnError):
        lib.gather_rows(torch.zeros(2, 4), torch.zeros(2, 4), t[:2])


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under fgnn-artifacts_amd/ may reference it."""
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "fgnn-artifacts_amd")):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cc", ".cpp")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                # (comments may CITE the oracle; code may not include, import, link or load it)
                if re.search(r"oracle_py|libfgnn_oracle|#\s*include\s*[<\"][^>\"]*oracle|import\s+oracle|from\s+oracle",
                             txt):
                    bad.append(os.path.join(dp, fn))
    assert not bad, bad


ENGINE_LIB = os.path.join(ROOT, "fgnn-artifacts_amd", "samgraph", "torch", "c_lib.so")


def test_engine_library_is_also_the_reference_named_python_module():
    """The reference's c_lib is ONE shared object: the samgraph_* C ABI for ctypes plus a Python module with the nine
    tensor getters (samgraph/torch/adapter.cc:177-189, imported by adapter.py:26).  Same here -- and without making the
    C-ABI library depend on libpython: no undefined Py* symbol, the CPython entry points are looked up when the
    interpreter calls PyInit_c_lib."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from samgraph.torch import c_lib
    want = ["samgraph_torch_get_graph_feat", "samgraph_torch_get_graph_label", "samgraph_torch_get_graph_row",
            "samgraph_torch_get_graph_col", "samgraph_torch_get_graph_data", "samgraph_torch_get_dataset_feat",
            "samgraph_torch_get_dataset_label", "samgraph_torch_get_graph_input_nodes",
            "samgraph_torch_get_graph_output_nodes"]
    assert all(callable(getattr(c_lib, n, None)) for n in want)
    assert os.path.samefile(c_lib.__file__, ENGINE_LIB)
    undefined = subprocess.run(["nm", "-D", "-u", ENGINE_LIB], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\b_?Py[A-Z_]", undefined), undefined
    # the zero-copy host wrapper used by get_dataset_feat / get_dataset_label
    import numpy as np
    a = np.arange(12, dtype=np.float32)
    t = c_lib._wrap(a.ctypes.data, 3, 4, 0, -1)
    assert t.shape == (3, 4) and t.data_ptr() == a.ctypes.data and float(t[2, 3]) == 11.0
    assert c_lib._wrap(0, 0, -1, 6, -1).shape == (0,)


def test_engine_library_loads_into_a_plain_c_host(tmp_path):
    """a C program (no Python in the process) dlopen()s c_lib.so with RTLD_NOW and finds the boundary's entry points"""
    src = tmp_path / "host.c"
    src.write_text("""
#include <dlfcn.h>
#include <stdio.h>
int main(int argc, char **argv) {
  void *h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "%s\\n", dlerror()); return 1; }
  const char *names[] = {"samgraph_config", "samgraph_init", "samgraph_get_next_batch", "samgraph_sample_once",
                         "samgraph_torch_get_graph_feat_ptr", "PyInit_c_lib"};
  for (unsigned i = 0; i < sizeof(names) / sizeof(names[0]); ++i)
    if (!dlsym(h, names[i])) { fprintf(stderr, "missing %s\\n", names[i]); return 2; }
  puts("ok");
  return 0;
}
""")
    exe = tmp_path / "host"
    subprocess.check_call(["gcc", "-O0", "-o", str(exe), str(src), "-ldl"])
    p = subprocess.run([str(exe), ENGINE_LIB], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr


def test_shipped_kernel_library_reads_no_switch_from_the_environment():
    """A stray FGNN_* variable must not change -- let alone corrupt -- a run: the shipped libfgnn_hip.so holds no such
    name at all (A/B switches and ablation masks exist only in the profiling build, csrc/Makefile `prof`,
    -DFGNN_PROFILING: fgnn_device.h tune_int).  (getenv itself stays imported: rocPRIM's headers, used at init time by
    presample.hip / prefix_tree.hip / the stateless weighted entry points, read their own variables.)"""
    from fgnn_hip import lib
    data = open(lib.LIB_PATH, "rb").read()
    assert b"FGNN_" not in data, "an FGNN_* name is compiled into the shipped library"


def test_shipped_engine_library_holds_no_test_switch():
    """c_lib.so reads the reference's SAMGRAPH_* variables plus a few of its own (documented in INTEGRATION.md); none of
    them may be a test hook -- the hand-off check's failure path is exercised from outside the engine (the hooks
    library flips a word of a published message, tests/test_engine_gpu.py) -- or swap / tune the kernel library."""
    data = open(ENGINE_LIB, "rb").read()
    for name in (b"SELFTEST", b"FGNN_HIP_LIB", b"corrupt", b"FGNN_TEST"):
        assert name not in data, "%r is compiled into the shipped engine library" % name
    # and it knows none of the profiling build's A/B switches
    for name in (b"FGNN_GATHER_", b"FGNN_FUSED_", b"FGNN_KHOP", b"FGNN_HT_", b"FGNN_SPLIT_", b"FGNN_PREFIX_TREE"):
        assert name not in data, name
