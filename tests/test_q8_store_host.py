"""CPU-only: the 8-bit feature store off the GPU -- `fgnn_dataset feat-q8` and the synthetic writer against the numpy
encode of tests/q8_refs.py byte for byte, fgnn_q8_row_bytes, and the config value feat_store_dtype = q8 through
fgnn_host_feat_store_probe (RunConfig::Parse and Dataset::Load)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import q8_refs as Q
from test_f16_store_host import ROOT, _probe, _write, data, tool  # noqa: F401  (the f16 store's fixtures and probe)

U8 = 3


# the last case holds more rows than one slice of the tool (2^22 / 64 = 65536), not a multiple of it
@pytest.mark.parametrize("rows,dim", [(9, 1), (9, 15), (9, 16), (9, 17), (40, 128), (9, 256), (70001, 64)])
def test_feat_q8_equals_the_numpy_encode_byte_for_byte(tool, tmp_path, rows, dim):  # noqa: F811
    feat = Q.features(rows, dim, seed=dim) if rows < 100 else \
        np.random.default_rng(1).standard_normal((rows, dim)).astype(np.float32)
    assert (feat[rows // 2] == feat[rows // 2, 0]).all() or rows > 100   # a constant row: scale 0, codes 0
    _write(str(tmp_path), feat)
    p = subprocess.run([tool, "feat-q8", str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    S = Q.row_bytes(dim)
    assert C.CDLL(os.path.join(ROOT, "fgnn-artifacts_amd", "lib", "libfgnn_hip.so")).fgnn_q8_row_bytes(C.c_size_t(dim)) == S
    got = np.fromfile(os.path.join(str(tmp_path), "feat_q8.bin"), dtype=np.uint8)
    want = Q.encode(feat)
    assert got.tobytes() == want.tobytes()
    assert not want[:, dim:S - 16].any() and not want[:, S - 8:].any()


def test_q8_store_maps_its_file_names_the_subcommand_without_it_and_sizes_empty_feat(data, tool, tmp_path):  # noqa: F811
    S = Q.row_bytes(12)
    p, out = _probe(data, feat_store_dtype="q8")
    assert p.returncode == -6 and out is None
    assert "feat_q8.bin" in p.stderr and "fgnn_dataset feat-q8" in p.stderr
    d = str(tmp_path / "g")
    shutil.copytree(data, d)
    assert subprocess.run([tool, "feat-q8", d], capture_output=True).returncode == 0
    p, out = _probe(d, feat_store_dtype="q8")
    assert p.returncode == 0 and out == [U8, 1, 500 * S, 1], p.stderr
    p, out = _probe(data, env={"SAMGRAPH_EMPTY_FEAT": "10"}, feat_store_dtype="q8")
    assert p.returncode == 0 and out == [U8, 1, 1024 * S, 0], p.stderr


def test_synthetic_writer_can_add_the_q8_table(tmp_path):
    from fgnn_hip import synth
    d = synth.write_dataset(str(tmp_path), "g", 300, 2000, 8, 4, 30, 5, 5, seed=4, feat_q8=True)
    feat = np.fromfile(os.path.join(d, "feat.bin"), dtype=np.float32).reshape(300, 8)
    assert np.fromfile(os.path.join(d, "feat_q8.bin"), dtype=np.uint8).tobytes() == Q.encode(feat).tobytes()
