"""CPU-only: the half-precision feature store off the GPU -- `fgnn_dataset feat-f16` against numpy's astype(float16)
byte for byte, the config key feat_store_dtype through the C ABI (include/fgnn_engine_hooks.h:
fgnn_host_feat_store_probe runs RunConfig::Parse and Dataset::Load), and the synthetic writers' option."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "dataset", "fgnn_dataset")
HOOKS = os.path.join(ROOT, "fgnn-artifacts_amd", "samgraph", "torch", "fgnn_engine_hooks.so")
F32, F16 = 0, 2


@pytest.fixture(scope="module")
def tool():
    src = TOOL + ".cc"
    if not os.path.exists(TOOL) or os.path.getmtime(TOOL) < os.path.getmtime(src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-o", TOOL, src], check=True)
    return TOOL


def _table(rows=64, dim=24):
    """f32 [rows, dim] holding normal values, values that round to fp16 subnormals (and to zero), ties of every kind,
    +-0, NaNs, the largest half, the largest float that still rounds to it, and infinities"""
    rs = np.random.default_rng(5)
    t = rs.standard_normal((rows, dim)).astype(np.float32)
    t[1] = (rs.standard_normal(dim) * 1e-6).astype(np.float32)                     # subnormal halves
    t[2] = (rs.standard_normal(dim) * 3e-8).astype(np.float32)                     # around the smallest subnormal
    # ties: exactly between two normal halves (even and odd neighbours), between two subnormals, 2^-25 (-> 0), 3 * 2^-25
    t[3, :8] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2048 + 1, 2048 + 3, 2.0 ** -25, 3 * 2.0 ** -25,
                5 * 2.0 ** -25]
    t[3, 8:12] = [2.0 ** -14 - 2.0 ** -25, 2.0 ** -14, np.float32(2.0 ** -14) * np.float32(1 - 2.0 ** -24), 2.0 ** -24]
    t[4, :6] = [0.0, -0.0, np.nan, -np.nan, 65504.0, -65504.0]
    t[4, 6] = np.nextafter(np.float32(65520.0), np.float32(0))                      # 65519.996: the last one that fits
    t[4, 7:9] = [np.inf, -np.inf]
    t[5] = np.frombuffer(rs.integers(0, 2 ** 32, dim, dtype=np.uint32).tobytes(), dtype=np.float32)  # any bit pattern
    t[5] = np.where(np.abs(t[5]) >= 65520, np.float32(1.5), t[5])                  # (NaNs stay: payloads are kept)
    t[6, :4].view(np.uint32)[:] = [0x7f800001, 0xffc00000, 0x7fa00000, 0x7f801fff]  # NaN payloads, one that would vanish
    return t


def _write(d, feat):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("NUM_NODE %d\nNUM_EDGE 0\nFEAT_DIM %d\nNUM_CLASS 2\nNUM_TRAIN_SET 0\nNUM_VALID_SET 0\nNUM_TEST_SET 0\n"
                % feat.shape)
    feat.tofile(os.path.join(d, "feat.bin"))


def test_feat_f16_equals_numpy_byte_for_byte(tool, tmp_path):
    d = str(tmp_path)
    feat = _table()
    assert np.isfinite(feat[np.isfinite(feat)].astype(np.float16)).all()
    _write(d, feat)
    p = subprocess.run([tool, "feat-f16", d], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "finite values that became infinite: 0" in p.stdout
    got = np.fromfile(os.path.join(d, "feat_f16.bin"), dtype=np.uint16)
    with np.errstate(over="ignore"):
        want = feat.astype(np.float16).view(np.uint16).ravel()
    assert got.tobytes() == want.tobytes()
    half = got.view(np.float16)
    assert (np.abs(half[np.isfinite(half)]) == 65504).sum() >= 3 and np.isnan(half).sum() >= 6
    assert ((half != 0) & (np.abs(half.astype(np.float64)) < 2.0 ** -14)).any()


def test_feat_f16_counts_overflows_and_refuses_them_unless_allowed(tool, tmp_path):
    d = str(tmp_path)
    feat = _table()
    feat[7, :3] = [65520.0, -1e9, 65519.99]   # two overflow (65520 is the tie that rounds up), the third fits
    _write(d, feat)
    p = subprocess.run([tool, "feat-f16", d], capture_output=True, text=True)
    assert p.returncode != 0 and "finite values that became infinite: 2" in p.stdout and "--allow-inf" in p.stderr
    assert not os.path.exists(os.path.join(d, "feat_f16.bin"))
    p = subprocess.run([tool, "feat-f16", d, "--allow-inf"], capture_output=True, text=True)
    assert p.returncode == 0 and "finite values that became infinite: 2" in p.stdout, p.stderr
    with np.errstate(over="ignore"):
        want = feat.astype(np.float16)
    assert np.fromfile(os.path.join(d, "feat_f16.bin"), dtype=np.uint16).tobytes() == want.tobytes()
    assert np.isinf(want[7, :2]).all() and want[7, 2] == 65504


def test_feat_f16_works_in_slices(tool, tmp_path):
    """more elements than one slice of the tool (2^22), not a multiple of it"""
    d = str(tmp_path)
    feat = np.random.default_rng(1).standard_normal((70001, 64)).astype(np.float32)
    _write(d, feat)
    assert subprocess.run([tool, "feat-f16", d], capture_output=True).returncode == 0
    assert np.fromfile(os.path.join(d, "feat_f16.bin"), dtype=np.uint16).tobytes() == feat.astype(np.float16).tobytes()


# ---- the config key, through the C ABI -----------------------------------------------------------------------------------

PROBE = ("import ctypes as C, sys\nL=C.CDLL(%r)\ncfg=%r\nk=[str(x).encode() for x in cfg]\n"
         "v=[str(x).encode() for x in cfg.values()]\no=(C.c_size_t*4)()\n"
         "L.fgnn_host_feat_store_probe((C.c_char_p*len(k))(*k),(C.c_char_p*len(v))(*v),C.c_size_t(len(k)),o)\n"
         "print('PROBE', *list(o))\n")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import synth
    return synth.write_dataset(str(tmp_path_factory.mktemp("store")), "g", 500, 3000, 12, 5, 40, 10, 10, seed=2)


def _probe(path, env=None, **over):
    """the probe in a process of its own (a failed check aborts; the shared regions die with the process)"""
    cfg = dict(dataset_path=path, _arch=1, _sample_type=5, batch_size=16, num_epoch=1, _cache_policy=2,
               cache_percentage=0.0, max_sampling_jobs=1, max_copying_jobs=1, omp_thread_num=2, sampler_ctx="cuda:0",
               trainer_ctx="cuda:0", num_fanout=2, fanout="3 2")
    cfg.update(over)
    e = {k: v for k, v in os.environ.items() if k not in ("SAMGRAPH_EMPTY_FEAT", "SAMGRAPH_SHM_PREFIX")}
    e.update(env or {})
    p = subprocess.run([sys.executable, "-c", PROBE % (HOOKS, cfg)], capture_output=True, text=True, env=e, timeout=120)
    out = [line for line in p.stdout.splitlines() if line.startswith("PROBE")]
    return p, ([int(x) for x in out[0].split()[1:]] if out else None)


def test_hook_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fgnn_engine_hooks.h")).read()
    assert "int fgnn_host_feat_store_probe(" in hdr and hasattr(C.CDLL(HOOKS), "fgnn_host_feat_store_probe")


def test_default_store_is_f32_from_feat_bin(data):
    p, out = _probe(data)
    assert p.returncode == 0 and out == [F32, 4, 500 * 12 * 4, 1], p.stderr
    p, out = _probe(data, feat_store_dtype="f32")
    assert p.returncode == 0 and out == [F32, 4, 500 * 12 * 4, 1], p.stderr


def test_unknown_value_is_a_config_error(data):
    for bad in ("bf16", "F16", "", "2"):
        p, out = _probe(data, feat_store_dtype=bad)
        assert p.returncode == -6 and out is None, (bad, p.stderr)  # SIGABRT, like every config error
        assert "eng_config.cc:" in p.stderr and "feat_store_dtype" in p.stderr


def test_f16_without_the_file_fails_and_names_the_subcommand(data):
    assert not os.path.exists(os.path.join(data, "feat_f16.bin"))
    p, out = _probe(data, feat_store_dtype="f16")
    assert p.returncode == -6 and out is None
    assert "feat_f16.bin" in p.stderr and "fgnn_dataset feat-f16" in p.stderr


def test_f16_maps_the_file_and_empty_feat_is_two_bytes_per_element(data, tool, tmp_path):
    import shutil
    d = str(tmp_path / "g")
    shutil.copytree(data, d)
    assert subprocess.run([tool, "feat-f16", d], capture_output=True).returncode == 0
    p, out = _probe(d, feat_store_dtype="f16")
    assert p.returncode == 0 and out == [F16, 2, 500 * 12 * 2, 1], p.stderr
    # SAMGRAPH_EMPTY_FEAT=k: a dummy region of 2^k rows, no file read -- at the store's element size
    p, out = _probe(d, env={"SAMGRAPH_EMPTY_FEAT": "10"}, feat_store_dtype="f16")
    assert p.returncode == 0 and out == [F16, 2, 1024 * 12 * 2, 0], p.stderr
    p, out = _probe(d, env={"SAMGRAPH_EMPTY_FEAT": "10"})
    assert p.returncode == 0 and out == [F32, 4, 1024 * 12 * 4, 0], p.stderr
    # ... and needs no file
    p, out = _probe(data, env={"SAMGRAPH_EMPTY_FEAT": "10"}, feat_store_dtype="f16")
    assert p.returncode == 0 and out == [F16, 2, 1024 * 12 * 2, 0], p.stderr


def test_synthetic_writer_can_add_the_half_table(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "fgnn-artifacts_amd"))
    from fgnn_hip import synth
    d = synth.write_dataset(str(tmp_path), "g", 300, 2000, 8, 4, 30, 5, 5, seed=4, feat_f16=True)
    feat = np.fromfile(os.path.join(d, "feat.bin"), dtype=np.float32)
    assert np.fromfile(os.path.join(d, "feat_f16.bin"), dtype=np.uint16).tobytes() == feat.astype(np.float16).tobytes()
    d2 = synth.write_dataset(str(tmp_path), "h", 300, 2000, 8, 4, 30, 5, 5, seed=4)
    assert not os.path.exists(os.path.join(d2, "feat_f16.bin"))
