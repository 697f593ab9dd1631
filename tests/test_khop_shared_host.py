"""Sample type khop_shared (8) in the host-side layers: Python names, exports and binding, run configuration."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_names():
    import samgraph.common as sc
    import samgraph.torch as sam
    from fgnn_hip import lib
    assert sc.kKHopShared == lib.KHOP_SHARED == 8
    # the reference's dict is left as the reference has it; the name is offered next to it
    assert sam.ext_sample_types == {"khop_shared": 8} and "khop_shared" not in sam.sample_types
    assert sam.all_sample_types == dict(sam.sample_types, khop_shared=8)
    L = lib.load()  # the exports and the binding table carry the new functions
    assert lib.SIGNATURES["fgnn_sample_khop_shared"] == lib.SIGNATURES["fgnn_sample_khop0"]
    assert lib.SIGNATURES["fgnn_khop_shared_scratch_bytes"] == (lib._Z, (lib._Z, lib._Z))
    for name in ("fgnn_sample_khop_shared", "fgnn_khop_shared_scratch_bytes", "fgnn_khop_shared_params"):
        assert hasattr(L, name) and name in lib.EXPORTS
    p = lib.khop_shared_params()
    assert p["max_fanout"] >= 64 and 64 < p["wave_row"] < p["block_row"]


def _configure(fanout):
    code = ("import sys; sys.path.insert(0, %r); import samgraph.torch as sam\n"
            "sam.config(dict(dataset_path='/nonexistent', _arch=sam.kArch1, _sample_type=sam.kKHopShared, batch_size=8,"
            " num_epoch=2, _cache_policy=sam.kCacheByDegree, cache_percentage=0.0, max_sampling_jobs=1,"
            " max_copying_jobs=1, omp_thread_num=1, sampler_ctx='cuda:0', trainer_ctx='cuda:0', num_fanout=2,"
            " fanout=[5, %d]))\nprint('accepted', sam.num_epoch())" % (os.path.join(ROOT, "fgnn-artifacts_amd"), fanout))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)


def test_run_config_accepts_the_type_and_refuses_a_fanout_above_the_limit():
    from fgnn_hip import lib
    limit = lib.khop_shared_params()["max_fanout"]
    ok = _configure(limit)
    assert ok.returncode == 0 and "accepted 2" in ok.stdout, ok.stdout + ok.stderr[-2000:]
    bad = _configure(limit + 1)
    assert bad.returncode != 0 and "khop_shared: fanout %d > %d" % (limit + 1, limit) in bad.stderr, bad.stderr[-2000:]
