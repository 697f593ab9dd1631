"""ctypes binding of fgnn-artifacts_amd/lib/libfgnn_hip.so (include/fgnn_hip.h).

PyTorch is used only as the owner of device memory and streams: every call below takes torch CUDA
(ROCm) tensors, passes their raw device pointers through the C ABI and enqueues HIP kernels on the
current torch stream.  There is NO fallback: if the library is missing, or no GPU is present, the
calls raise.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library.  Nothing in the environment changes which file is loaded: the measurement tools under tools/ that
# want the profiling build (lib/libfgnn_hip_prof.so, `make -C csrc prof`: the only build whose kernels read A/B switches
# and ablation masks) say so in their own code, with use_library(path), before anything calls load()
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libfgnn_hip.so")
PROF_LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libfgnn_hip_prof.so")


def use_library(path):
    """tools/ only: bind another build of the kernel library (before the first call of load())."""
    global LIB_PATH
    if _lib is not None:
        raise FgnnError("use_library() after the kernel library has been loaded")
    LIB_PATH = os.path.abspath(path)


SRC_GLOBAL, SRC_LOCAL = 0, 1
LINK_WGS_SHARED, LINK_WGS_DEDICATED = 16, 16  # FGNN_LINK_WGS_* (fgnn_hip.h)
EMPTY = 0xFFFFFFFF
F32, F64, F16, U8, I32, I8, I64 = range(7)
_T2DT = {torch.float32: F32, torch.float64: F64, torch.float16: F16, torch.uint8: U8, torch.int32: I32,
         torch.int8: I8, torch.int64: I64}

_lib = None

# Every function include/fgnn_hip.h declares: return type, argument types, derived from the prototype by rule
# (tests/test_binding_signatures.py compares the two).  Any pointer, array, handle, structure pointer or stream is a
# c_void_p -- it takes an int address, None, a c_void_p, byref(x) or a ctypes array -- and a scalar is its ctypes twin,
# so the call sites pass addresses and plain numbers.  load() applies the table; nothing else types a function.
_P, _S, _I, _U, _Z, _U32, _U64 = C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.c_size_t, C.c_uint32, C.c_uint64
_LL, _ULL, _F, _D = C.c_longlong, C.c_ulonglong, C.c_float, C.c_double
SIGNATURES = {
    "fgnn_version": (_S, ()),
    "fgnn_last_error": (_S, ()),
    "fgnn_device_count": (_I, ()),
    "fgnn_debug_phase_log_bytes": (_Z, ()),
    "fgnn_debug_phase_log": (None, (_P,)),
    "fgnn_debug_occupy": (_I, (_Z, _U, _P)),
    "fgnn_debug_random_reads": (_I, (_P, _Z, _Z, _U64, _P, _P)),
    "fgnn_debug_scan_helps": (_ULL, ()),
    "fgnn_debug_set_scan_help_after": (None, (_I,)),
    "fgnn_debug_set_partition_lds_limit": (None, (_I,)),
    "fgnn_debug_partition_params": (None, (_P,)),
    "fgnn_debug_gather_plan": (_I, (_Z, _Z, _I, _I, _U32, _Z, _Z, _I, _P, _Z)),
    "fgnn_debug_sort_pairs": (_I, (_P, _P, _Z, _P)),
    "fgnn_debug_scan_block_sums": (_I, (_P, _Z, _P, _P, _P, _P, _P, _P, _U32, _P)),
    "fgnn_debug_scan_count": (_I, (_I, _P)),
    "fgnn_debug_scan_set": (_I, (_I, _P, _LL, _LL)),
    "fgnn_debug_scan_get": (_I, (_I, _P, _I, _P)),
    "fgnn_debug_set_stateless_ticket_start_once": (None, (_U32,)),
    "fgnn_scratch_bytes": (_Z, (_Z,)),
    "fgnn_sanity_map_bytes": (_Z, (_Z,)),
    "fgnn_sanity_check_batch": (_I, (_P, _Z, _P, _Z, _U32, _P, _P)),
    "fgnn_sample_khop0": (_I, (_P, _P, _P, _Z, _P, _Z, _Z, _P, _P, _P, _I, _U64, _U64, _U32, _P, _Z, _P)),
    "fgnn_sample_khop2": (_I, (_P, _P, _P, _Z, _P, _Z, _Z, _P, _P, _P, _I, _U64, _U64, _U32, _P, _Z, _P)),
    "fgnn_weighted_scratch_bytes": (_Z, (_Z, _Z)),
    "fgnn_sample_weighted_khop_prefix": (_I, (_P, _P, _P, _P, _Z, _P, _Z, _Z, _P, _P, _P, _I, _U64, _U64, _U32, _P, _Z,
                                            _P)),
    "fgnn_sample_khop1": (_I, (_P, _P, _P, _Z, _P, _Z, _Z, _P, _P, _P, _I, _U64, _U64, _U32, _P, _Z, _P)),
    "fgnn_sample_weighted_khop": (_I, (_P, _P, _P, _P, _P, _Z, _P, _Z, _Z, _P, _P, _P, _I, _U64, _U64, _U32, _P, _Z,
                                     _P)),
    "fgnn_hash_dedup_scratch_bytes": (_Z, (_Z,)),
    "fgnn_sample_weighted_khop_hash_dedup": (_I, (_P, _P, _P, _P, _P, _Z, _P, _Z, _Z, _P, _P, _P, _I, _U64, _U64, _U32,
                                                _P, _Z, _P)),
    "fgnn_random_walk_scratch_bytes": (_Z, (_Z, _Z)),
    "fgnn_sample_random_walk": (_I, (_P, _P, _P, _Z, _P, _Z, _Z, _D, _Z, _Z, _P, _P, _P, _P, _I, _U64, _U64, _U32, _P,
                                   _Z, _P)),
    "fgnn_extract_neighbour_scratch_bytes": (_Z, (_Z,)),
    "fgnn_extract_neighbour": (_I, (_P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _Z, _P)),
    "fgnn_neighbourhood_expand": (_I, (_P, _P, _P, _Z, _P, _Z, _P, _U32, _P, _P, _Z, _P, _I, _P)),
    "fgnn_hashtable_create": (_P, (_Z, _P)),
    "fgnn_hashtable_create_ex": (_P, (_Z, _Z, _P)),
    "fgnn_hashtable_destroy": (None, (_P,)),
    "fgnn_hashtable_capacity": (_Z, (_P,)),
    "fgnn_hashtable_reset": (_I, (_P, _P)),
    "fgnn_hashtable_fill_unique": (_I, (_P, _P, _Z, _P)),
    "fgnn_hashtable_fill_duplicates": (_I, (_P, _P, _Z, _P, _Z, _P, _P, _Z, _P)),
    "fgnn_hashtable_map": (_I, (_P, _P, _Z, _P, _Z, _P, _P)),
    "fgnn_hashtable_set_n2o": (_I, (_P, _P)),
    "fgnn_hashtable_start_batch": (_I, (_P, _P, _Z, _P, _P, _U64, _U32, _P)),
    "fgnn_hashtable_n2o": (_P, (_P,)),
    "fgnn_hashtable_d_num_items": (_P, (_P,)),
    "fgnn_get_miss_cache_index": (_I, (_P, _P, _Z, _P, _Z, _P, _P, _P, _P, _P, _P, _Z, _P)),
    "fgnn_cache_table_replace": (_I, (_P, _P, _Z, _P, _Z, _P)),
    "fgnn_gather_rows": (_I, (_P, _P, _P, _P, _Z, _P, _Z, _Z, _I, _P)),
    "fgnn_gather_rows_masked": (_I, (_P, _P, _P, _P, _Z, _P, _Z, _Z, _I, _U32, _P)),
    "fgnn_gather_rows_shared": (_I, (_P, _P, _P, _P, _Z, _P, _Z, _Z, _I, _U32, _I, _P)),
    "fgnn_extract_fused": (_I, (_P, _P)),
    "fgnn_extract_fused_grid": (_Z, (_P,)),
    "fgnn_extract_fused_link_grid": (_Z, (_P,)),
    "fgnn_block_aggregate": (_I, (_P, _P, _P, _Z, _P, _Z, _P, _P)),
    "fgnn_block_aggregate_ex": (_I, (_P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P)),
    "fgnn_block_degrees": (_I, (_P, _P, _P, _Z, _P, _P, _P)),
    "fgnn_block_aggregate_scaled": (_I, (_P, _P, _P, _Z, _P, _Z, _Z, _P, _Z, _P, _I, _P, _I, _P)),
    "fgnn_block_aggregate_ex_f16": (_I, (_P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P)),
    "fgnn_block_aggregate_scaled_f16": (_I, (_P, _P, _P, _Z, _P, _Z, _Z, _P, _Z, _P, _I, _P, _I, _P)),
    "fgnn_csr_split_length": (_Z, ()),
    "fgnn_csr_aggregate_workspace_bytes": (_Z, (_Z, _Z, _Z)),
    "fgnn_csr_aggregate": (_I, (_P, _P, _P, _P, _Z, _Z, _Z, _P, _Z, _Z, _P, _Z, _P, _I, _P, _I, _P, _Z, _P)),
    "fgnn_csr_aggregate_f16": (_I, (_P, _P, _P, _P, _Z, _Z, _Z, _P, _Z, _Z, _P, _Z, _P, _I, _P, _I, _P, _Z, _P)),
    "fgnn_csr_gat_max_heads": (_Z, ()),
    "fgnn_csr_gat_workspace_bytes": (_Z, (_Z, _Z, _Z, _Z)),
    "fgnn_csr_gat_attention": (_I, (_P, _P, _P, _Z, _Z, _Z, _P, _P, _P, _Z, _Z, _Z, _F, _P, _Z, _P, _Z, _P)),
    "fgnn_relu_l2norm": (_I, (_P, _Z, _P, _Z, _P, _Z, _Z, _P)),
    "fgnn_relu_l2norm_backward": (_I, (_P, _Z, _P, _P, _Z, _P, _Z, _Z, _Z, _P)),
    "fgnn_gat_workspace_bytes": (_Z, (_Z, _Z, _Z)),
    "fgnn_gat_forward": (_I, (_P, _P, _Z, _P, _P, _P, _Z, _Z, _Z, _Z, _F, _F, _U64, _P, _U32, _P, _P, _Z, _P, _Z, _P)),
    "fgnn_gat_backward": (_I, (_P, _P, _Z, _P, _P, _P, _Z, _P, _P, _Z, _Z, _Z, _Z, _F, _F, _U64, _P, _U32, _P, _Z, _P,
                             _P, _P, _Z, _P)),
    "fgnn_sage_finish_z": (_I, (_P, _Z, _P, _Z, _P, _P, _Z, _Z, _P)),
    "fgnn_sage_finish_z_f16": (_I, (_P, _Z, _P, _Z, _P, _P, _Z, _Z, _P)),
    "fgnn_sage_grad_prep": (_I, (_P, _Z, _P, _P, _P, _Z, _Z, _Z, _P)),
    "fgnn_relu_dropout": (_I, (_P, _P, _Z, _F, _U64, _P, _U32, _P)),
    "fgnn_relu_dropout_backward": (_I, (_P, _P, _P, _Z, _F, _P)),
    "fgnn_softmax_xent_scratch_bytes": (_Z, (_Z,)),
    "fgnn_softmax_xent": (_I, (_P, _Z, _P, _Z, _Z, _P, _P, _Z, _P, _Z, _P)),
    "fgnn_adam_step": (_I, (_P, _P, _P, _P, _P, _I, _F, _F, _F, _F, _F, _P, _P)),
    "fgnn_presample_count": (_I, (_P, _P, _Z, _P, _Z, _P)),
    "fgnn_presample_rank_scratch_bytes": (_Z, (_Z,)),
    "fgnn_presample_rank": (_I, (_P, _Z, _P, _P, _Z, _P)),
    "fgnn_cache_table_build": (_I, (_P, _Z, _P, _Z, _P)),
    "fgnn_sampler_create": (_P, (_P, _P)),
    "fgnn_sampler_destroy": (None, (_P,)),
    "fgnn_sampler_prefix_tree_stats": (_I, (_P, _P)),
    "fgnn_sampler_max_nodes": (_Z, (_P,)),
    "fgnn_sampler_max_edges": (_Z, (_P, _I)),
    "fgnn_batch_create": (_P, (_P, _Z, _I, _I, _Z, _P)),
    "fgnn_batch_destroy": (None, (_P,)),
    "fgnn_sampler_sample": (_I, (_P, _P, _Z, _U64, _P, _P)),
    "fgnn_sampler_sample_indexed": (_I, (_P, _P, _Z, _U64, _P, _P, _P)),
    "fgnn_sampler_sample_ordered": (_I, (_P, _U64, _P, _Z, _U64, _P, _P)),
    "fgnn_sampler_sample_begin": (_I, (_P, _P, _Z, _U64, _P, _P, _P)),
    "fgnn_sampler_sample_begin_ordered": (_I, (_P, _U64, _P, _Z, _U64, _P, _P)),
    "fgnn_sampler_sample_end": (_I, (_P, _U64, _P, _P, _P)),
    "fgnn_sampler_run_batch": (_I, (_P, _U64, _P, _Z, _U64, _P, _P, _P, _P, _P)),
    "fgnn_sampler_run_range": (_I, (_P, _P, _U64, _Z, _P, _P, _P)),
    "fgnn_batch_cache_index": (_I, (_P, _P, _P)),
    "fgnn_batch_set_feat_row_mask": (_I, (_P, _U32)),
    "fgnn_batch_extract": (_I, (_P, _P, _P, _P)),
    "fgnn_batch_extract_cached": (_I, (_P, _P, _P, _P, _P)),
    "fgnn_sampler_run_batch_cached": (_I, (_P, _U64, _P, _Z, _U64, _P, _P, _P, _P, _P, _P)),
    "fgnn_batch_extract_cached_ms": (_I, (_P, _P)),
    "fgnn_batch_extract_launch_ms": (_F, (_P,)),
    "fgnn_batch_enable_timing": (_I, (_P, _I)),
    "fgnn_batch_gather_ms": (_F, (_P,)),
    "fgnn_batch_gather_kernel_ms": (_F, (_P,)),
    "fgnn_batch_finish": (_I, (_P, _P)),
    "fgnn_batch_host_meta": (_P, (_P,)),
    "fgnn_batch_meta_copied": (_I, (_P,)),
    "fgnn_batch_wait": (_I, (_P, _P)),
    "fgnn_batch_row": (_P, (_P, _I)),
    "fgnn_batch_col": (_P, (_P, _I)),
    "fgnn_batch_data": (_P, (_P, _I)),
    "fgnn_batch_input_nodes": (_P, (_P,)),
    "fgnn_batch_output_nodes": (_P, (_P,)),
    "fgnn_batch_feat": (_P, (_P,)),
    "fgnn_batch_label": (_P, (_P,)),
    "fgnn_batch_cache_index_ptr": (_P, (_P, _I)),
    "fgnn_batch_device_meta": (_P, (_P,)),
}
EXPORTS = list(SIGNATURES)


class DebugScanState(C.Structure):
    """fgnn_debug_scan_state (fgnn_hip.h)"""
    _fields_ = [("gen", C.c_uint32), ("ticket_base", C.c_uint32), ("ticket_word", C.c_uint32), ("wipes", C.c_uint32),
                ("max_desc_gen", C.c_uint32), ("max_tiles", C.c_uint32)]


SCAN_OF_SAMPLER, SCAN_OF_HASHTABLE, SCAN_OF_BATCH = 0, 1, 2  # FGNN_DEBUG_SCAN_OF_*
SCAN_GEN_LIMIT = 0x3FFFFFFE  # the last generation of a cycle: the launch after it wipes the descriptors and carries 1

# fgnn_debug_partition_params: names of out[0 .. 8), in order
PARTITION_PARAMS = ("min_log2", "max_log2", "per_bin", "lds_slots", "lds_limit", "reg_items", "hopeless_items", "tile")


class FgnnError(RuntimeError):
    pass


def load():
    """Loads the HIP library; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FgnnError(f"{LIB_PATH} is missing: build it with `make -C fgnn-artifacts_amd/csrc` "
                            "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        # (neither the library nor this binding reads a switch from the environment: tests that force the helping path of
        # the single-pass kernels call fgnn_debug_set_scan_help_after themselves, tests/conftest.py)
        _lib = L
    return _lib


def _check(code, what):
    if code != 0:
        detail = load().fgnn_last_error().decode() if code == -3 else ""
        raise FgnnError(f"{what} failed with code {code} {detail}")


class DevicePointer:
    """a raw device-visible address standing in for a tensor argument (registered host memory whose device address is
    not its host address); `keep` holds whatever owns the memory"""

    def __init__(self, address, keep=None):
        self.address, self.keep = int(address), keep

    def data_ptr(self):
        return self.address

    is_cuda = True


def _ptr(t):
    """device-visible address of a tensor or a DevicePointer; None (a null pointer) for None"""
    return t.data_ptr() if t is not None else None


def _stream(t=None):
    """handle of the current stream of the current device, or, given a tensor, of that tensor's device"""
    return torch.cuda.current_stream(t.device if t is not None else None).cuda_stream


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise FgnnError("fgnn_hip kernels need device tensors (no CPU fallback)")


def _as_u32(t):
    """uint32 storage viewed through torch.int32 (torch has no native uint32 arithmetic)."""
    assert t.dtype in (torch.int32, torch.uint32) and t.is_contiguous()
    return t


def scratch(n_cap, device):
    return torch.empty(load().fgnn_scratch_bytes(int(n_cap)), dtype=torch.uint8, device=device)


def sample_khop(kind, indptr, indices, inp, fanout, seed, batch_key, layer, src_mode=SRC_GLOBAL, d_num_input=None,
                ws=None):
    """kind in {'khop0','khop2'}.  Returns (out_src, out_dst, d_num_out) -- device tensors, sized for the
    worst case num_input*fanout; d_num_out is an int64[1] device scalar.  Asynchronous."""
    L = load()
    _need_gpu(indptr, indices, inp)
    n = inp.numel()
    dev = inp.device
    out_src = torch.empty(max(n * fanout, 1), dtype=torch.int32, device=dev)
    out_dst = torch.empty(max(n * fanout, 1), dtype=torch.int32, device=dev)
    d_num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    if ws is None:
        ws = scratch(n, dev)
        if kind == "khop0":  # room for the hub tables: rows beyond 16 K entries are then drawn by the whole chip
            ws = torch.empty(ws.numel() + 4 * (n + 16 + 1024 * (fanout + 3)), dtype=torch.uint8, device=dev)
    fn = L.fgnn_sample_khop0 if kind == "khop0" else L.fgnn_sample_khop2
    code = fn(_ptr(indptr), _ptr(indices), _ptr(inp), n, _ptr(d_num_input), n, fanout, _ptr(out_src), _ptr(out_dst),
              _ptr(d_num_out), src_mode, seed, batch_key, layer, _ptr(ws), ws.numel(), _stream())
    _check(code, "fgnn_sample_" + kind)
    return out_src, out_dst, d_num_out


def debug_sort_pairs(keys, vals):
    """fgnn_debug_sort_pairs: (keys, vals) int32 CUDA tensors sorted in place by key (as uint32), stable."""
    _need_gpu(keys, vals)
    assert keys.numel() == vals.numel()
    _check(load().fgnn_debug_sort_pairs(_ptr(keys), _ptr(vals), keys.numel(), _stream()), "fgnn_debug_sort_pairs")


def _scan_handle(obj):
    kind = (SCAN_OF_SAMPLER if isinstance(obj, Sampler) else SCAN_OF_HASHTABLE if isinstance(obj, HashTable) else
            SCAN_OF_BATCH if isinstance(obj, Batch) else None)
    if kind is None:
        raise FgnnError("a Sampler, a HashTable or a Batch owns look-back descriptors; %r does not" % (obj,))
    return kind, obj.h


def debug_scan_set(obj, gen=-1, ticket=-1):
    """fgnn_debug_scan_set: host generation and / or ticket counter (device word and host base) of every look-back
    descriptor set that `obj` (Sampler, HashTable, Batch) owns; -1 leaves a counter alone.  Synchronises."""
    kind, h = _scan_handle(obj)
    _check(load().fgnn_debug_scan_set(kind, h, gen, ticket), "fgnn_debug_scan_set")


def debug_scan_states(obj):
    """fgnn_debug_scan_get for every descriptor set of `obj`: a list of DebugScanState.  Synchronises."""
    kind, h = _scan_handle(obj)
    L = load()
    n = L.fgnn_debug_scan_count(kind, h)
    if n < 0:
        _check(n, "fgnn_debug_scan_count")
    out = []
    for i in range(n):
        st = DebugScanState()
        _check(L.fgnn_debug_scan_get(kind, h, i, C.byref(st)), "fgnn_debug_scan_get")
        out.append(st)
    return out


def debug_partition_params():
    """fgnn_debug_partition_params: {name: value} of the partitioned fill's compiled-in constants (PARTITION_PARAMS).
    Needs no GPU."""
    out = (C.c_uint32 * len(PARTITION_PARAMS))()
    load().fgnn_debug_partition_params(out)
    return dict(zip(PARTITION_PARAMS, (int(v) for v in out)))


def debug_gather_plan(rows, row_bytes, device_sized=False, has_src_index=True, src_row_mask=0xFFFFFFFF, cus=256,
                      wg_per_cu=4, unroll=4, max_launches=4096):
    """fgnn_debug_gather_plan: the launches a gather of `rows` rows of row_bytes would be made of, as a list of
    (first_row, rows, grid, tile), or None where the library refuses the gather (FGNN_EINVAL).  Needs no GPU."""
    out = (C.c_uint64 * (4 * max(max_launches, 1)))()
    rc = load().fgnn_debug_gather_plan(rows, row_bytes, int(device_sized), int(has_src_index), src_row_mask, cus,
                                       wg_per_cu, unroll, out, max_launches)
    if rc == -1:
        return None
    if rc < 0:
        _check(rc, "fgnn_debug_gather_plan")
    return [tuple(int(v) for v in out[4 * k:4 * k + 4]) for k in range(rc)]


def debug_scan_block_sums(sums, n=None, total64=None, total32=None, accum=None, accum_out=None, items32=None,
                          items64=None, items_per_sum=0):
    """fgnn_debug_scan_block_sums: the one-workgroup exclusive scan of scan.hip on device tensors (int32 storage for
    uint32 words, int64[1] for total64 / items64), in place; waits."""
    _need_gpu(sums, total64, total32, accum, accum_out, items32, items64)
    n = sums.numel() if n is None else n
    _check(load().fgnn_debug_scan_block_sums(_ptr(sums) if n else None, n, _ptr(total64), _ptr(total32), _ptr(accum),
                                             _ptr(accum_out), _ptr(items32), _ptr(items64), items_per_sum, _stream()),
           "fgnn_debug_scan_block_sums")


def sample_weighted_khop_prefix(indptr, indices, prefix, inp, fanout, seed, batch_key, layer, src_mode=SRC_GLOBAL,
                                d_num_input=None):
    L = load()
    _need_gpu(indptr, indices, prefix, inp)
    n, dev = inp.numel(), inp.device
    out_src = torch.empty(max(n * fanout, 1), dtype=torch.int32, device=dev)
    out_dst = torch.empty(max(n * fanout, 1), dtype=torch.int32, device=dev)
    d_num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.fgnn_weighted_scratch_bytes(max(n, 1), fanout), dtype=torch.uint8, device=dev)
    _check(L.fgnn_sample_weighted_khop_prefix(_ptr(indptr), _ptr(indices), _ptr(prefix), _ptr(inp), n,
                                              _ptr(d_num_input), n, fanout, _ptr(out_src), _ptr(out_dst),
                                              _ptr(d_num_out), src_mode, seed, batch_key, layer, _ptr(ws), ws.numel(),
                                              _stream()), "fgnn_sample_weighted_khop_prefix")
    return out_src, out_dst, d_num_out


def sample_with_replacement(kind, indptr, indices, inp, fanout, seed, batch_key, layer, prob=None, alias=None,
                            src_mode=SRC_GLOBAL):
    """kind in {'khop1', 'weighted_khop' (alias method), 'weighted_khop_hash_dedup'}."""
    L = load()
    _need_gpu(indptr, indices, inp)
    n, dev = inp.numel(), inp.device
    out_src = torch.empty(max(n * fanout, 1), dtype=torch.int32, device=dev)
    out_dst = torch.empty(max(n * fanout, 1), dtype=torch.int32, device=dev)
    d_num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.fgnn_weighted_scratch_bytes(max(n, 1), fanout), dtype=torch.uint8, device=dev)
    tail = (_ptr(inp), n, None, n, fanout, _ptr(out_src), _ptr(out_dst), _ptr(d_num_out), src_mode, seed, batch_key,
            layer, _ptr(ws), ws.numel(), _stream())
    if kind == "khop1":
        _check(L.fgnn_sample_khop1(_ptr(indptr), _ptr(indices), *tail), "fgnn_sample_khop1")
    elif kind == "weighted_khop_hash_dedup":
        _check(L.fgnn_sample_weighted_khop_hash_dedup(_ptr(indptr), _ptr(indices), _ptr(prob), _ptr(alias), *tail),
               "fgnn_sample_weighted_khop_hash_dedup")
    else:
        _check(L.fgnn_sample_weighted_khop(_ptr(indptr), _ptr(indices), _ptr(prob), _ptr(alias), *tail),
               "fgnn_sample_weighted_khop")
    return out_src, out_dst, d_num_out


def sample_random_walk(indptr, indices, inp, walk_len, restart_prob, num_walks, K, seed, batch_key, layer,
                       src_mode=SRC_GLOBAL, d_num_input=None):
    L = load()
    _need_gpu(indptr, indices, inp)
    n, dev = inp.numel(), inp.device
    outs = [torch.empty(max(n * K, 1), dtype=torch.int32, device=dev) for _ in range(3)]
    d_num_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.fgnn_random_walk_scratch_bytes(max(n, 1), K), dtype=torch.uint8, device=dev)
    _check(L.fgnn_sample_random_walk(_ptr(indptr), _ptr(indices), _ptr(inp), n, _ptr(d_num_input), n, walk_len,
                                     restart_prob, num_walks, K, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                     _ptr(d_num_out), src_mode, seed, batch_key, layer, _ptr(ws), ws.numel(), _stream()),
           "fgnn_sample_random_walk")
    return outs[0], outs[1], outs[2], d_num_out


class HashTable:
    """OrderedHashTable (cuda_hashtable.h:99-149) on the GPU."""

    def __init__(self, max_items, device="cuda:0", max_fill_items=None):
        """max_fill_items: largest fill_duplicates call; when given, reset() is a generation bump (see fgnn_hip.h)."""
        L = load()
        torch.cuda.set_device(device)
        err = C.c_int(0)
        if max_fill_items is None:
            self.h = L.fgnn_hashtable_create(max_items, C.byref(err))
        else:
            self.h = L.fgnn_hashtable_create_ex(max_items, max_fill_items, C.byref(err))
        if not self.h:
            raise FgnnError(f"fgnn_hashtable_create failed with code {err.value}")
        self.max_items = max_items
        self.device = torch.device(device)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.fgnn_hashtable_destroy(self.h)
            self.h = None

    def reset(self):
        _check(load().fgnn_hashtable_reset(self.h, _stream()), "fgnn_hashtable_reset")

    def fill_unique(self, items):
        _need_gpu(items)
        _check(load().fgnn_hashtable_fill_unique(self.h, _ptr(items), items.numel(), _stream()),
               "fgnn_hashtable_fill_unique")

    def fill_duplicates(self, items, num_items=None, d_num_items=None, want_mapped=True, ws=None):
        """Returns mapped (int32 device tensor, local id per item) or None."""
        _need_gpu(items)
        cap = items.numel()
        n = cap if num_items is None else num_items
        mapped = torch.empty(max(cap, 1), dtype=torch.int32, device=items.device) if want_mapped else None
        if ws is None:
            ws = scratch(cap, items.device)
        _check(load().fgnn_hashtable_fill_duplicates(self.h, _ptr(items), n, _ptr(d_num_items), cap, _ptr(mapped),
                                                     _ptr(ws), ws.numel(), _stream()), "fgnn_hashtable_fill_duplicates")
        return mapped

    def map(self, items):
        _need_gpu(items)
        mapped = torch.empty(max(items.numel(), 1), dtype=torch.int32, device=items.device)
        _check(load().fgnn_hashtable_map(self.h, _ptr(items), items.numel(), None, items.numel(), _ptr(mapped),
                                         _stream()), "fgnn_hashtable_map")
        return mapped[:items.numel()]

    def capacity(self):
        """buckets of the table: the power of two >= max(1024, 2 * max_items)"""
        return int(load().fgnn_hashtable_capacity(self.h))

    def num_items(self):
        """Synchronises."""
        p = load().fgnn_hashtable_d_num_items(self.h)
        t = _wrap_device_u32(p, 1, self.device)
        return int(t.cpu()[0])

    def d_num_items_ptr(self):
        return load().fgnn_hashtable_d_num_items(self.h)

    def unique(self, n=None):
        """Copy of the N2O list (first n entries; default all current items).  Synchronises if n is None."""
        if n is None:
            n = self.num_items()
        p = load().fgnn_hashtable_n2o(self.h)
        return _wrap_device_u32(p, n, self.device).clone()


class _DevArray:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _wrap_device_u32(ptr, n, device):
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=device)
    return torch.as_tensor(_DevArray(ptr, n, "<i4"), device=device)


def extract_neighbour(indptr, indices, inp, out_cap, num_input=None, d_num_input=None):
    """GPUExtractNeighbour: returns (out[out_cap], d_num_out int64[1]) device tensors.  Asynchronous."""
    L = load()
    _need_gpu(indptr, indices, inp)
    cap = inp.numel()
    n = cap if num_input is None else num_input
    dev = inp.device
    out = torch.empty(max(out_cap, 1), dtype=torch.int32, device=dev)
    d_num_out = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.fgnn_extract_neighbour_scratch_bytes(cap), dtype=torch.uint8, device=dev)
    _check(L.fgnn_extract_neighbour(_ptr(indptr), _ptr(indices), _ptr(inp), n, _ptr(d_num_input), cap, _ptr(out),
                                    out_cap, _ptr(d_num_out), _ptr(ws), ws.numel(), _stream()), "fgnn_extract_neighbour")
    return out, d_num_out


def neighbourhood_expand(indptr, indices, frontier, stamp, mark, freq, nxt, d_num_next, mark_frontier=False,
                         num_frontier=None, d_num_frontier=None):
    """One level of the closed-neighbourhood search (fgnn_neighbourhood_expand); d_num_next (int32[1]) is added to."""
    _need_gpu(indptr, indices, frontier, stamp, nxt, d_num_next)
    cap = frontier.numel()
    n = cap if num_frontier is None else num_frontier
    _check(load().fgnn_neighbourhood_expand(_ptr(indptr), _ptr(indices), _ptr(frontier), n, _ptr(d_num_frontier), cap,
                                            _ptr(stamp), mark, _ptr(freq), _ptr(nxt), nxt.numel(), _ptr(d_num_next),
                                            1 if mark_frontier else 0, _stream()), "fgnn_neighbourhood_expand")


class SanityChecker:
    """SAMGRAPH_SANITY_CHECK's per-epoch net (GPUSanityCheckList + GPUBatchSanityCheck, cuda_sanity_check.cu:28-88):
    check(batch) returns the flag word -- 0 = fine, 1 = an invalid id, 2 = an id seen before in this epoch (or twice in
    the batch), 4 = an id >= num_node.  new_epoch() clears the seen-bitmap."""

    def __init__(self, num_node, device, invalid_val=EMPTY):
        self.num_node, self.invalid = num_node, invalid_val
        self.bits = torch.zeros(load().fgnn_sanity_map_bytes(num_node) // 4, dtype=torch.int32, device=device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=device)

    def new_epoch(self):
        self.bits.zero_()

    def check(self, batch, no_duplicates=True):
        _need_gpu(batch)
        self.flags.zero_()
        _check(load().fgnn_sanity_check_batch(_ptr(self.bits) if no_duplicates else None, self.num_node, _ptr(batch),
                                              batch.numel(), self.invalid, _ptr(self.flags), _stream()),
               "fgnn_sanity_check_batch")
        return int(self.flags.item())


def presample_count(freq, nodes, num_nodes=None, d_num_nodes=None):
    """PreSampler's counting step: freq[nodes[i]] += 1 (dist/pre_sampler.cc:117-131).  Asynchronous."""
    _need_gpu(freq, nodes)
    cap = nodes.numel()
    n = cap if num_nodes is None else num_nodes
    _check(load().fgnn_presample_count(_ptr(freq), _ptr(nodes), n, _ptr(d_num_nodes), cap, _stream()),
           "fgnn_presample_count")


def presample_rank(freq):
    """rank list (int32 device tensor, u32 storage): nodes by (frequency desc, id desc) (dist/pre_sampler.cc:140-160)."""
    L = load()
    _need_gpu(freq)
    n = freq.numel()
    ws = torch.empty(L.fgnn_presample_rank_scratch_bytes(n), dtype=torch.uint8, device=freq.device)
    rank = torch.empty(n, dtype=torch.int32, device=freq.device)
    _check(L.fgnn_presample_rank(_ptr(freq), n, _ptr(rank), _ptr(ws), ws.numel(), _stream()), "fgnn_presample_rank")
    return rank


def cache_table_build(rank, num_cached, num_node=None):
    """direct-map table node -> cache slot (SampleCacheTableInit, dist_engine.cc:193-229)"""
    _need_gpu(rank)
    n = rank.numel() if num_node is None else num_node
    table = torch.empty(n, dtype=torch.int32, device=rank.device)
    _check(load().fgnn_cache_table_build(_ptr(table), n, _ptr(rank), num_cached, _stream()), "fgnn_cache_table_build")
    return table


def cache_table_replace(table, old_nodes, new_nodes):
    """ReplaceCacheGPU's index update: old nodes -> EMPTY, new node i -> i"""
    _need_gpu(table, old_nodes, new_nodes)
    n_old = 0 if old_nodes is None else old_nodes.numel()
    _check(load().fgnn_cache_table_replace(_ptr(table), _ptr(old_nodes) if n_old else None, n_old, _ptr(new_nodes),
                                           new_nodes.numel(), _stream()), "fgnn_cache_table_replace")


def get_miss_cache_index(table, nodes, num_nodes=None, d_num_nodes=None, ws=None):
    """Returns (miss_src, miss_dst, cache_src, cache_dst, d_counts[2]) device tensors sized len(nodes)."""
    _need_gpu(table, nodes)
    cap = nodes.numel()
    n = cap if num_nodes is None else num_nodes
    dev = nodes.device
    outs = [torch.empty(max(cap, 1), dtype=torch.int32, device=dev) for _ in range(4)]
    d_counts = torch.zeros(2, dtype=torch.int32, device=dev)
    if ws is None:
        ws = scratch(cap, dev)
    _check(load().fgnn_get_miss_cache_index(_ptr(table), _ptr(nodes), n, _ptr(d_num_nodes), cap, _ptr(outs[0]),
                                            _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(d_counts), _ptr(ws),
                                            ws.numel(), _stream()), "fgnn_get_miss_cache_index")
    return outs[0], outs[1], outs[2], outs[3], d_counts


def gather_rows(out, src, src_index=None, dst_index=None, n=None, d_n=None, src_row_mask=None, shared_gpu=None):
    """out[dst_index[i] or i] = src[(src_index[i] or i) & src_row_mask]; rows are the trailing dims.
    shared_gpu (not None): fgnn_gather_rows_shared -- a host-source launch stays small on a GPU that also samples."""
    _need_gpu(out)
    if n is None:
        n = (src_index if src_index is not None else dst_index if dst_index is not None else src).shape[0]
    dim = 1
    for s in out.shape[1:]:
        dim *= s
    assert out.dtype == src.dtype and out.is_contiguous() and src.is_contiguous()
    if shared_gpu is not None:
        mask = 0xFFFFFFFF if src_row_mask is None else src_row_mask
        _check(load().fgnn_gather_rows_shared(_ptr(out), _ptr(src), _ptr(src_index), _ptr(dst_index), n, _ptr(d_n), n,
                                              dim, _T2DT[out.dtype], mask, int(shared_gpu), _stream()),
               "fgnn_gather_rows_shared")
        return out
    if src_row_mask is not None:
        _check(load().fgnn_gather_rows_masked(_ptr(out), _ptr(src), _ptr(src_index), _ptr(dst_index), n, _ptr(d_n), n,
                                              dim, _T2DT[out.dtype], src_row_mask, _stream()), "fgnn_gather_rows_masked")
        return out
    _check(load().fgnn_gather_rows(_ptr(out), _ptr(src), _ptr(src_index), _ptr(dst_index), n, _ptr(d_n), n, dim,
                                   _T2DT[out.dtype], _stream()), "fgnn_gather_rows")
    return out


def random_read_rate(array, num_items=4_000_000, repeats=24):
    """independent random 4-byte reads per second the GPU sustains from `array` (an int32 device tensor far larger than
    the caches) right now: fgnn_debug_random_reads, `repeats` launches of num_items reads between two events"""
    _need_gpu(array)
    sink = torch.zeros(1, dtype=torch.int32, device=array.device)
    L = load()

    def launch(salt):
        _check(L.fgnn_debug_random_reads(_ptr(array), array.numel(), num_items, salt, _ptr(sink), _stream()),
               "fgnn_debug_random_reads")
    launch(1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(repeats):
        launch(2 + r * num_items)
    e1.record()
    e1.synchronize()
    return repeats * num_items / (e0.elapsed_time(e1) * 1e-3)


class CopySegment(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("words", C.c_size_t)]


class ExtractJob(C.Structure):
    """fgnn_extract_job (include/fgnn_hip.h)"""
    _fields_ = [("out", C.c_void_p), ("miss_rows", C.c_void_p), ("cache_rows", C.c_void_p),
                ("miss_src", C.c_void_p), ("miss_dst", C.c_void_p), ("cache_src", C.c_void_p), ("cache_dst", C.c_void_p),
                ("num_miss", C.c_size_t), ("num_cache", C.c_size_t), ("d_counts", C.c_void_p), ("cap", C.c_size_t),
                ("dim", C.c_size_t), ("dtype", C.c_int), ("miss_row_mask", C.c_uint32),
                ("label_out", C.c_void_p), ("label_src", C.c_void_p), ("label_index", C.c_void_p),
                ("num_label", C.c_size_t), ("label_dtype", C.c_int),
                ("segs", C.POINTER(CopySegment)), ("num_segs", C.c_int), ("link_workgroups", C.c_int),
                ("stamps", C.c_void_p)]


def extract_fused(out, miss_rows, cache_rows, miss_src, miss_dst, cache_src, cache_dst, num_miss=None, num_cache=None,
                  d_counts=None, miss_row_mask=0xFFFFFFFF, label_out=None, label_src=None, label_index=None,
                  copies=(), link_workgroups=0, stamps=None):
    """fgnn_extract_fused: out[miss_dst] = miss_rows[miss_src & mask], out[cache_dst] = cache_rows[cache_src], the label
    rows and the word copies `copies` = [(dst, src, words)] in ONE launch.  Counts: host values (default: the index
    lists' lengths) or d_counts = device {num_miss, num_cache}.  Returns (workgroups, link-band workgroups)."""
    _need_gpu(out)
    dim = 1
    for s in out.shape[1:]:
        dim *= s
    j = ExtractJob()
    j.out, j.miss_rows, j.cache_rows = _ptr(out), _ptr(miss_rows), _ptr(cache_rows)
    j.miss_src, j.miss_dst, j.cache_src, j.cache_dst = _ptr(miss_src), _ptr(miss_dst), _ptr(cache_src), _ptr(cache_dst)
    j.num_miss = (miss_src.numel() if miss_src is not None else 0) if num_miss is None else num_miss
    j.num_cache = (cache_src.numel() if cache_src is not None else 0) if num_cache is None else num_cache
    if d_counts is not None:
        j.d_counts = _ptr(d_counts)
        j.cap = max(miss_src.numel() if miss_src is not None else 0, cache_src.numel() if cache_src is not None else 0)
    j.dim, j.dtype, j.miss_row_mask = dim, _T2DT[out.dtype], miss_row_mask
    if label_out is not None:
        j.label_out, j.label_src, j.label_index = _ptr(label_out), _ptr(label_src), _ptr(label_index)
        j.num_label, j.label_dtype = label_index.numel(), _T2DT[label_out.dtype]
    segs = (CopySegment * max(len(copies), 1))()
    for k, (d, s, words) in enumerate(copies):
        segs[k].dst, segs[k].src, segs[k].words = _ptr(d), _ptr(s), words
    j.segs, j.num_segs = segs, len(copies)
    j.link_workgroups = link_workgroups
    j.stamps = _ptr(stamps)
    L = load()
    _check(L.fgnn_extract_fused(C.byref(j), _stream()), "fgnn_extract_fused")
    return int(L.fgnn_extract_fused_grid(C.byref(j))), int(L.fgnn_extract_fused_link_grid(C.byref(j)))


# ---------------------------------------------------------------------------------------------------
# batch driver (fgnn_sampler / fgnn_batch)

MAX_LAYERS = 8
KHOP0, KHOP1, WEIGHTED_KHOP, RANDOM_WALK, WEIGHTED_KHOP_PREFIX, KHOP2, WEIGHTED_KHOP_HASH_DEDUP = 0, 1, 2, 3, 4, 5, 6


class SamplerConfig(C.Structure):
    _fields_ = [("indptr", C.c_void_p), ("indices", C.c_void_p), ("prob_prefix", C.c_void_p),
                ("num_node", C.c_size_t), ("sample_type", C.c_int), ("num_layers", C.c_size_t),
                ("fanout", C.c_size_t * MAX_LAYERS), ("max_batch_size", C.c_size_t), ("seed", C.c_uint64),
                ("walk_len", C.c_size_t), ("num_walks", C.c_size_t), ("restart_prob", C.c_double),
                ("prob_table", C.c_void_p), ("alias_table", C.c_void_p)]


class RunPlan(C.Structure):
    _fields_ = [("d_train", C.c_void_p), ("num_train", C.c_size_t), ("batch_size", C.c_size_t),
                ("batches", C.c_void_p), ("num_batches", C.c_size_t), ("streams", C.c_void_p),
                ("num_streams", C.c_size_t), ("cache_table", C.c_void_p), ("feat", C.c_void_p), ("label", C.c_void_p),
                ("cached", C.c_int), ("cache_rows", C.c_void_p), ("full_feat", C.c_void_p)]


class BatchMeta(C.Structure):
    _fields_ = [("key", C.c_uint64), ("num_edge", C.c_uint64 * MAX_LAYERS), ("num_src", C.c_uint32 * MAX_LAYERS),
                ("num_dst", C.c_uint32 * MAX_LAYERS), ("num_layers", C.c_uint32), ("num_input", C.c_uint32),
                ("num_output", C.c_uint32), ("num_miss", C.c_uint32), ("num_cache", C.c_uint32),
                ("overflow", C.c_uint32), ("t_start", C.c_uint64), ("t_sampled", C.c_uint64), ("t_closed", C.c_uint64)]


_TORCH_OF = {F32: torch.float32, F64: torch.float64, F16: torch.float16, U8: torch.uint8, I32: torch.int32,
             I8: torch.int8, I64: torch.int64}
_TYPESTR = {F32: "<f4", F64: "<f8", F16: "<f2", U8: "|u1", I32: "<i4", I8: "|i1", I64: "<i8"}


def _wrap_device(ptr, shape, dtype_code, device):
    n = 1
    for s in shape:
        n *= s
    if n == 0:
        return torch.empty(shape, dtype=_TORCH_OF[dtype_code], device=device)

    class _A:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": _TYPESTR[dtype_code], "data": (ptr, False),
                                    "version": 2}
    return torch.as_tensor(_A(), device=device)


class Sampler:
    """DoGPUSample / DoGetCacheMissIndex / DoGPUFeatureExtract on one GPU, no host round trips."""

    def __init__(self, indptr, indices, fanout, max_batch_size, sample_type=KHOP2, seed=0x5A4D47, prob_prefix=None,
                 walk_len=0, num_walks=0, restart_prob=0.0, prob_table=None, alias_table=None):
        L = load()
        _need_gpu(indptr, indices)
        self.device = indptr.device
        torch.cuda.set_device(self.device)
        self._keep = (indptr, indices, prob_prefix, prob_table, alias_table)
        cfg = SamplerConfig()
        cfg.indptr, cfg.indices, cfg.prob_prefix = _ptr(indptr), _ptr(indices), _ptr(prob_prefix)
        cfg.num_node = indptr.numel() - 1
        cfg.sample_type = sample_type
        cfg.num_layers = len(fanout)
        for i, f in enumerate(fanout):
            cfg.fanout[i] = f
        cfg.max_batch_size, cfg.seed = max_batch_size, seed
        cfg.walk_len, cfg.num_walks, cfg.restart_prob = walk_len, num_walks, restart_prob
        cfg.prob_table, cfg.alias_table = _ptr(prob_table), _ptr(alias_table)
        if prob_prefix is not None:
            torch.cuda.synchronize(self.device)  # the sampler reads the table while it is created (search trees)
        err = C.c_int(0)
        self.h = L.fgnn_sampler_create(C.byref(cfg), C.byref(err))
        if not self.h:
            raise FgnnError(f"fgnn_sampler_create failed with code {err.value} {L.fgnn_last_error().decode()}")
        self.fanout = list(fanout)
        self.max_batch_size = max_batch_size
        self.max_nodes = L.fgnn_sampler_max_nodes(self.h)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.fgnn_sampler_destroy(self.h)
            self.h = None

    def prefix_tree_stats(self):
        """(rows with a search tree, long rows refused as not non-decreasing, bytes) -- weighted_khop_prefix only"""
        out = (C.c_size_t * 3)()
        _check(load().fgnn_sampler_prefix_tree_stats(self.h, out), "fgnn_sampler_prefix_tree_stats")
        return int(out[0]), int(out[1]), int(out[2])

    def max_edges(self, layer):
        return load().fgnn_sampler_max_edges(self.h, layer)

    def new_batch(self, feat_dim=0, feat_dtype=F32, label_dtype=I64, feat_rows_cap=0):
        return Batch(self, feat_dim, feat_dtype, label_dtype, feat_rows_cap)

    def sample(self, seeds, batch_key, batch, seq=None):
        """seq=None: internal call counter (single-threaded use); else the explicit batch order (thread-safe)."""
        _need_gpu(seeds)
        if seq is None:
            _check(load().fgnn_sampler_sample(self.h, _ptr(seeds), seeds.numel(), batch_key, batch.h, _stream()),
                   "fgnn_sampler_sample")
        else:
            _check(load().fgnn_sampler_sample_ordered(self.h, seq, _ptr(seeds), seeds.numel(), batch_key, batch.h,
                                                      _stream()), "fgnn_sampler_sample_ordered")

    def sample_indexed(self, seeds, batch_key, batch, cache_table=None):
        """fgnn_sampler_sample_indexed: sample + cache index in one call (an arch5 sampler's batch), internal counter"""
        _need_gpu(seeds)
        _check(load().fgnn_sampler_sample_indexed(self.h, _ptr(seeds), seeds.numel(), batch_key, batch.h,
                                                  _ptr(cache_table), _stream()), "fgnn_sampler_sample_indexed")

    def sample_begin(self, seq, seeds, batch_key, batch, stream=None):
        """fgnn_sampler_sample_begin_ordered: the batch's sampling CHAIN (everything up to its last sampler launch).
        Enqueue begin(k + 1) before end(k) to keep khop2's cross-batch chain busy; `stream` of end = that of begin."""
        _need_gpu(seeds)
        st = (stream or torch.cuda.current_stream()).cuda_stream
        _check(load().fgnn_sampler_sample_begin_ordered(self.h, seq, _ptr(seeds), seeds.numel(), batch_key, batch.h, st),
               "fgnn_sampler_sample_begin_ordered")

    def sample_end(self, seq, batch, cache_table=None, stream=None):
        """fgnn_sampler_sample_end: the batch's TAIL (last dedup fill, fix-ups, table reset) [+ the cache-index split];
        extraction / finish are the caller's, on the same stream"""
        st = (stream or torch.cuda.current_stream()).cuda_stream
        _check(load().fgnn_sampler_sample_end(self.h, seq, batch.h, _ptr(cache_table), st), "fgnn_sampler_sample_end")

    def run_batch(self, seq, seeds, batch_key, batch, cache_table=None, feat=None, label=None, stream=None):
        """sample + cache index + extract + finish in ONE C call on `stream` (a torch stream; default current).
        Safe to call from several Python threads (ctypes releases the GIL)."""
        _need_gpu(seeds)
        st = (stream or torch.cuda.current_stream()).cuda_stream
        _check(load().fgnn_sampler_run_batch(self.h, seq, _ptr(seeds), seeds.numel(), batch_key, batch.h,
                                             _ptr(cache_table), _ptr(feat), _ptr(label), st), "fgnn_sampler_run_batch")

    def run_range(self, first_seq, count, train, batch_size, batches, streams, cache_table=None, feat=None, label=None,
                  cache_rows=None, full_feat=None, cached=False):
        """fgnn_sampler_run_range: batches first_seq .. first_seq+count-1 enqueued and collected by ONE native call (the
        reference's C++ loop thread, cuda_loops_arch1.cc:38-84).  Returns (metas, times, host_enqueue_seconds); times[i]
        = (ms, ms) HIP-event times of batch i, -1 where not timed.  Raises on a flagged batch."""
        call = self.range_call(first_seq, count, train, batch_size, batches, streams, cache_table, feat, label,
                               cache_rows, full_feat, cached)
        call.run()
        return call.results()

    def range_call(self, first_seq, count, train, batch_size, batches, streams, cache_table=None, feat=None,
                   label=None, cache_rows=None, full_feat=None, cached=False):
        """run_range in three steps for callers that time the native call alone: the argument marshalling here,
        .run() = the one C call (returns when every batch of the range has been collected), .results() afterwards."""
        _need_gpu(train)
        return _RangeCall(self, first_seq, count, train, batch_size, batches, streams, cache_table, feat, label,
                          cache_rows, full_feat, cached)

    def run_batch_cached(self, seq, seeds, batch_key, batch, cache_table, cache_rows, full_feat, label=None,
                         stream=None):
        """sample + cache index + CombineMissData (rows read from `full_feat`: device or pinned host tensor) +
        CombineCacheData + finish in one C call."""
        _need_gpu(seeds, cache_table, cache_rows)
        st = (stream or torch.cuda.current_stream()).cuda_stream
        _check(load().fgnn_sampler_run_batch_cached(self.h, seq, _ptr(seeds), seeds.numel(), batch_key, batch.h,
                                                    _ptr(cache_table), _ptr(cache_rows), _ptr(full_feat), _ptr(label),
                                                    st), "fgnn_sampler_run_batch_cached")


class _RangeCall:
    def __init__(self, sampler, first_seq, count, train, batch_size, batches, streams, cache_table, feat, label,
                 cache_rows, full_feat, cached):
        self.L = load()
        self.sampler, self.first_seq, self.count, self.batches = sampler, first_seq, count, batches
        plan = self.plan = RunPlan()
        plan.d_train, plan.num_train, plan.batch_size = train.data_ptr(), train.numel(), batch_size
        self._keep = (train, cache_table, feat, label, cache_rows, full_feat, list(streams),
                      (C.c_void_p * len(batches))(*[b.h for b in batches]),
                      (C.c_void_p * len(streams))(*[st.cuda_stream for st in streams]))
        plan.batches, plan.num_batches = C.cast(self._keep[-2], C.c_void_p), len(batches)
        plan.streams, plan.num_streams = C.cast(self._keep[-1], C.c_void_p), len(streams)
        plan.cache_table, plan.feat, plan.label = _ptr(cache_table), _ptr(feat), _ptr(label)
        plan.cached = 1 if cached else 0
        plan.cache_rows, plan.full_feat = _ptr(cache_rows), _ptr(full_feat)
        self.metas = (BatchMeta * max(count, 1))()
        self.times = (C.c_float * (2 * max(count, 1)))()
        self.busy = C.c_double(0.0)
        self.rc = None
        self._args = (sampler.h, C.byref(plan), first_seq, count, self.metas, self.times, C.byref(self.busy))

    def run(self):
        self.rc = self.L.fgnn_sampler_run_range(*self._args)

    def results(self):
        _check(self.rc, "fgnn_sampler_run_range")
        count, batches = self.count, self.batches
        out = [self.metas[i] for i in range(count)]
        for m in out:
            if m.overflow:
                raise FgnnError(f"batch {m.key} is invalid (overflow flag {m.overflow})")
        for i in range(max(0, count - len(batches)), count):  # the buffers hold the last batches: views stay usable
            batches[(self.first_seq + i) % len(batches)].meta = out[i]
        return out, [(self.times[2 * i], self.times[2 * i + 1]) for i in range(count)], self.busy.value


class Batch:
    def __init__(self, sampler, feat_dim, feat_dtype, label_dtype, feat_rows_cap):
        L = load()
        err = C.c_int(0)
        self.sampler = sampler
        self.h = L.fgnn_batch_create(sampler.h, feat_dim, feat_dtype, label_dtype, feat_rows_cap, C.byref(err))
        if not self.h:
            raise FgnnError(f"fgnn_batch_create failed with code {err.value} {L.fgnn_last_error().decode()}")
        self.feat_dim, self.feat_dtype, self.label_dtype = feat_dim, feat_dtype, label_dtype
        self.feat_rows_cap = min(feat_rows_cap, sampler.max_nodes) if feat_rows_cap else sampler.max_nodes
        self.meta = None
        self._views = {}

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.fgnn_batch_destroy(self.h)
            self.h = None

    def cache_index(self, table):
        _check(load().fgnn_batch_cache_index(self.h, _ptr(table), _stream()), "fgnn_batch_cache_index")

    def extract(self, feat=None, label=None):
        _check(load().fgnn_batch_extract(self.h, _ptr(feat), _ptr(label), _stream()), "fgnn_batch_extract")

    def extract_cached(self, cache_rows, full_feat, label=None):
        _check(load().fgnn_batch_extract_cached(self.h, _ptr(cache_rows), _ptr(full_feat), _ptr(label), _stream()),
               "fgnn_batch_extract_cached")

    def finish(self):
        _check(load().fgnn_batch_finish(self.h, _stream()), "fgnn_batch_finish")

    def enable_timing(self, on=True):
        _check(load().fgnn_batch_enable_timing(self.h, 1 if on else 0), "fgnn_batch_enable_timing")

    def gather_ms(self):
        return float(load().fgnn_batch_gather_ms(self.h))

    def extract_cached_ms(self):
        """(miss-row gather ms, cached-row gather ms) of the last extract_cached, -1 where not timed"""
        out = (C.c_float * 2)()
        _check(load().fgnn_batch_extract_cached_ms(self.h, out), "fgnn_batch_extract_cached_ms")
        return float(out[0]), float(out[1])

    def extract_launch_ms(self):
        """HIP-event time around the whole one-launch cached extraction (-1 when not timed)"""
        return float(load().fgnn_batch_extract_launch_ms(self.h))

    def d_num_input(self):
        """device view (int32[1]) of the batch summary's num_input"""
        p = load().fgnn_batch_device_meta(self.h)
        return _wrap_device_u32(p + BatchMeta.num_input.offset, 1, self.sampler.device)

    def input_nodes_buffer(self):
        """the whole input_nodes buffer (capacity max_nodes); valid entries = num_input"""
        return _wrap_device_u32(load().fgnn_batch_input_nodes(self.h), self.sampler.max_nodes, self.sampler.device)

    def wait(self):
        m = BatchMeta()
        _check(load().fgnn_batch_wait(self.h, C.byref(m)), "fgnn_batch_wait")
        self.meta = m
        if m.overflow:
            raise FgnnError(f"batch {m.key} is invalid (overflow flag {m.overflow}): a capacity was exceeded or a "
                            "cross-workgroup wait timed out")
        return m

    # views of the device buffers, sized by the (waited-for) summary.  A buffer of the batch never moves: it is wrapped
    # ONCE at its full capacity (torch.as_tensor on a __cuda_array_interface__ object costs ~25 us, eight of them per
    # batch were a fifth of a training step's host time) and every call returns a slice of that tensor.
    def _whole(self, key, ptr_fn, shape, dtype_code):
        t = self._views.get(key)
        if t is None:
            t = self._views[key] = _wrap_device(ptr_fn(), shape, dtype_code, self.sampler.device)
        return t

    def graph(self, layer):
        m, L = self.meta, load()
        ne, cap = int(m.num_edge[layer]), self.sampler.max_edges(layer)
        row = self._whole(("row", layer), lambda: L.fgnn_batch_row(self.h, layer), (cap,), I32)[:ne]
        col = self._whole(("col", layer), lambda: L.fgnn_batch_col(self.h, layer), (cap,), I32)[:ne]
        return row, col, int(m.num_src[layer]), int(m.num_dst[layer])

    def graph_buffers(self, layer):
        """(row, col) of a layer at their full capacity (the buffers never move): for callers that need stable addresses
        and sizes, e.g. a captured graph (examples/graphed_step.py); valid entries = meta.num_edge[layer]"""
        L, cap = load(), self.sampler.max_edges(layer)
        return (self._whole(("row", layer), lambda: L.fgnn_batch_row(self.h, layer), (cap,), I32),
                self._whole(("col", layer), lambda: L.fgnn_batch_col(self.h, layer), (cap,), I32))

    def feat_buffer(self):
        """the feature buffer at its full capacity [feat_rows_cap, feat_dim]; valid rows = meta.num_input"""
        return self._whole("feat", lambda: load().fgnn_batch_feat(self.h), (self.feat_rows_cap, self.feat_dim),
                           self.feat_dtype)

    def graph_data(self, layer):
        L = load()
        if not L.fgnn_batch_data(self.h, layer):
            return None
        return self._whole(("data", layer), lambda: L.fgnn_batch_data(self.h, layer), (self.sampler.max_edges(layer),),
                           I32)[:int(self.meta.num_edge[layer])]

    def input_nodes(self):
        return self._whole("input", lambda: load().fgnn_batch_input_nodes(self.h), (self.sampler.max_nodes,),
                           I32)[:int(self.meta.num_input)]

    def output_nodes(self):
        return self._whole("output", lambda: load().fgnn_batch_output_nodes(self.h), (self.sampler.max_batch_size,),
                           I32)[:int(self.meta.num_output)]

    def feat(self):
        # a batch larger than a caller-chosen feat_rows_cap carries meta.overflow and only the first cap rows
        return self._whole("feat", lambda: load().fgnn_batch_feat(self.h), (self.feat_rows_cap, self.feat_dim),
                           self.feat_dtype)[:min(int(self.meta.num_input), self.feat_rows_cap)]

    def label(self):
        return self._whole("label", lambda: load().fgnn_batch_label(self.h), (self.sampler.max_batch_size,),
                           self.label_dtype)[:int(self.meta.num_output)]

    def cache_index_arrays(self):
        m, L = self.meta, load()
        n = [int(m.num_miss), int(m.num_miss), int(m.num_cache), int(m.num_cache)]
        return [self._whole(("cidx", k), lambda k=k: L.fgnn_batch_cache_index_ptr(self.h, k), (self.sampler.max_nodes,),
                            I32)[:n[k]] for k in range(4)]
