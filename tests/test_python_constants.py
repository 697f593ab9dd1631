"""samgraph.common must reproduce the reference's enum block (samgraph/common/__init__.py:47-265)."""
import json
import os

import pytest


def test_constants_match_reference(golden_dir):
    import samgraph.common as sc
    with open(os.path.join(golden_dir, "py_constants.json")) as f:
        ref = json.load(f)
    assert len(ref["constants"]) == 130
    for name, val in ref["constants"].items():
        assert getattr(sc, name) == val, name
    assert sc.sample_types == ref["sample_types"]
    assert sc.cache_policies == ref["cache_policies"]
    assert sc.builtin_archs == ref["builtin_archs"]
    assert sc.cpu(1) == "cpu:1" and sc.gpu(3) == "cuda:3"


@pytest.mark.parametrize("mode,argv", [
    ("NORMAL", []),                                          # defaults: arch3, khop0
    ("NORMAL", ["--arch", "arch2", "--sample-type", "khop2", "--cache-percentage", "0.1", "--pipeline"]),
    ("FGNN", ["--num-sample-worker", "2", "--num-train-worker", "3", "--cache-percentage", "0.2"]),
])
def test_reference_common_config_is_accepted_unchanged(tmp_path, golden_dir, mode, argv):
    """The run_config dict the reference's own CLI/config harness (example/samgraph/common_config.py) builds for these
    arguments with THIS repo's samgraph package behind `import samgraph.torch as sam`, as recorded in
    tests/golden/common_config_run_configs.json; samgraph_config must take the dict as it is (keys, value formats,
    unknown keys ignored), and the enum values the harness looked up by name are this package's."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(golden_dir, "common_config_run_configs.json")) as f:
        cases = json.load(f)["cases"]
    rc = next(c["run_config"] for c in cases if c["mode"] == mode and c["argv"] == argv)
    assert rc["fanout"] == [25, 10] and rc["num_fanout"] == rc["num_layer"] == 2
    code = r'''
import sys
sys.path.insert(0, %r)
import samgraph.torch as sam
rc = %r
assert rc["_arch"] == sam.builtin_archs[rc["arch"]]["arch"]
assert rc["_sample_type"] == sam.sample_types[rc["sample_type"]]
assert rc["_cache_policy"] == sam.cache_policies[rc["cache_policy"]]
sam.config(rc)
assert sam.num_epoch() == rc["num_epoch"]
print("accepted", rc["_arch"], rc["_sample_type"], rc["num_epoch"])
''' % (os.path.join(root, "fgnn-artifacts_amd"), rc)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode == 0 and "accepted" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]


def test_hardware_queue_default_is_set_before_the_first_hip_call():
    """An arch5 rank drives five HIP streams; the runtime's default of 4 hardware queues makes two batch streams take
    turns.  Importing the package sets GPU_MAX_HW_QUEUES=8 unless the user has set it."""
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os, sys; sys.path.insert(0, %r); os.environ.pop('GPU_MAX_HW_QUEUES', None); "
            "import samgraph.common; print(os.environ['GPU_MAX_HW_QUEUES'])" % os.path.join(ROOT, "fgnn-artifacts_amd"))
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True).stdout.strip() == "8"
    code = code.replace("os.environ.pop('GPU_MAX_HW_QUEUES', None)", "os.environ['GPU_MAX_HW_QUEUES'] = '5'")
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True).stdout.strip() == "5"
