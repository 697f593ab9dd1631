"""Every path of the feature-movement kernels (csrc/cache_gather.hip: fgnn_gather_rows / _masked / _shared,
fgnn_extract_fused with its label tail and word copies, the batch driver's extraction with other types than F32 / I64,
fgnn_get_miss_cache_index around its items-per-thread switch) against the numpy references of tests/gather_refs.py,
byte for byte.  Grid caps come from the device's CU count.  Every output is poisoned and has guard rows before and
after; rows that are no destination and the guards must come back unchanged.  Index entries beyond a device-side count
are valid row numbers whose destination is a guard row, so a kernel that reads past its count changes a guard instead
of faulting; no case addresses memory outside its buffers.  No gather is launched whose chunk total lies within
grid * tile of 2^32: that window is covered on the CPU (tests/test_gather_references.py) -- a library without the
admissibility rule never returns from such a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import gather_refs as G

pytestmark = pytest.mark.gpu
P, GR = G.POISON, G.GUARD_ROWS


@pytest.fixture(scope="module")
def hip():
    from fgnn_hip import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.fixture(scope="module")
def cus(hip):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bytes_on_device(a, off=0):
    """(tensor, address): the bytes of `a` on the device, `off` bytes behind a 16-byte boundary"""
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.empty(raw.size + 32, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    if raw.size:
        t[off:off + raw.size].copy_(torch.from_numpy(raw))
    return t, t.data_ptr() + off


def _back(t, off, like):
    return t[off:off + like.size].cpu().numpy().reshape(like.shape)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host_u32(t, n=None):
    a = t.cpu().numpy()
    return (a if n is None else a[:n]).view(np.uint32)


# ---- stand-alone gathers: the pairwise table ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", G.GATHER_CASES, ids=G.case_id)
def test_gather_case(hip, cus, case):
    lay = G.build_gather_case(case, cus)
    assert G.layout_stays_inside(lay)
    L = hip.load()
    src_t, src_p = _bytes_on_device(lay.src, lay.src_off)
    blank = np.full_like(lay.want, P)
    out_t, out_p = _bytes_on_device(blank, lay.out_off)
    body_p = out_p + lay.body * lay.row_bytes
    if lay.row_bytes % 16 == 0:  # whole-chunk rows reach the element kernel through a misaligned base only
        assert (body_p % 16 == 0 and src_p % 16 == 0) == (G.case_path(case) != "elem")
    idx_t = dev(lay.idx) if lay.idx is not None else None
    dst_t = dev(lay.dst) if lay.dst is not None else None
    dn_t = dev(np.array([lay.d_n], np.uint32)) if lay.d_n is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    args = (body_p, src_p, ptr(idx_t), ptr(dst_t), lay.n_host, ptr(dn_t), lay.cap, lay.dim, G.DTYPES[case.dtype][0])
    if case.mask == "none":
        rc = L.fgnn_gather_rows(*args, _stream())
    else:
        rc = L.fgnn_gather_rows_masked(*args, lay.mask, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = _back(out_t, lay.out_off, lay.want)
    assert got[:GR].tobytes() == lay.want[:GR].tobytes() and got[-GR:].tobytes() == lay.want[-GR:].tobytes(), "guard rows"
    assert got.tobytes() == lay.want.tobytes()
    assert lay.n == 0 or (lay.want != P).any()


@pytest.mark.parametrize("dim", [128, 3], ids=["512B-chunks", "12B-elements"])
@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("pinned", [True, False], ids=["pinned-host", "hbm"])
def test_shared_gpu_hint_with_host_and_hbm_sources(hip, dim, shared, pinned):
    rs = np.random.default_rng(7)
    n_src, n = 1 << 10, 5003
    src = rs.standard_normal((n_src, dim)).astype(np.float32)
    idx = rs.integers(0, 1 << 20, size=n).astype(np.uint32)
    dst = rs.permutation(n + 13)[:n].astype(np.uint32)
    want = np.full((GR + n + 13 + GR, dim * 4), P, np.uint8)
    G.gather_ref(want[GR:-GR], src.view(np.uint8).reshape(n_src, -1), n, idx, dst, n_src - 1)
    table = torch.from_numpy(src).pin_memory() if pinned else dev(src)
    out = torch.from_numpy(np.full_like(want, P)).cuda().view(torch.float32)
    hip.gather_rows(out[GR:-GR], table, src_index=dev(idx), dst_index=dev(dst), src_row_mask=n_src - 1, shared_gpu=shared)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()


# ---- fused extraction ----------------------------------------------------------------------------------------------------------

LABEL_TYPES = {1: (np.uint8, torch.uint8), 2: (np.float16, torch.float16), 4: (np.int32, torch.int32),
               8: (np.int64, torch.int64)}


def _segments(rs, count):
    """`count` word copies out of one source buffer into one destination buffer, at odd word offsets, every third of
    them empty: [(dst offset, src offset, words)], words of the two buffers"""
    sizes = [0 if k % 3 == 1 else int(s) for k, s in enumerate(rs.choice([1, 2, 255, 256, 257, 1000, 2049], size=count))]
    segs, d_at, s_at = [], 1, 3
    for w in sizes:
        segs.append((d_at, s_at, w))
        d_at += w + (2 if w % 2 == 0 else 1)  # keep every offset odd, leave a gap of poison
        s_at += w + (2 if w % 2 == 0 else 1)
    return segs, d_at + 8, s_at + 8


def _run_fused(hip, cpr, n_miss, n_cache, seed, counts="host", pad=0, link=0, host_rows=False, label=None, num_segs=0):
    """one fgnn_extract_fused launch laid out like the stand-alone cases, checked against gather_ref; returns
    (grid, link band)"""
    rs = np.random.default_rng(seed)
    rb = 16 * cpr
    miss_tab = rs.integers(0, 256, size=(64, rb), dtype=np.uint8)       # a 2^6-row table behind masked ids
    cache_tab = rs.integers(0, 256, size=(301, rb), dtype=np.uint8)
    cap_m, cap_c = (max(n_miss, n_cache) + pad,) * 2 if counts == "device" else (n_miss, n_cache)
    body = n_miss + n_cache + 13
    perm = rs.permutation(body).astype(np.uint32)
    ms = rs.integers(0, 1 << 20, size=cap_m).astype(np.uint32)
    cs = rs.integers(0, 301, size=cap_c).astype(np.uint32)
    ms[n_miss:], cs[n_cache:] = 64 * 7 + 2, 5                            # beyond the counts: valid rows ...
    md = np.concatenate([perm[:n_miss], body + np.arange(cap_m - n_miss, dtype=np.uint32) % GR]).astype(np.uint32)
    cd = np.concatenate([perm[n_miss:n_miss + n_cache],                  # ... whose destination is a guard row
                         body + np.arange(cap_c - n_cache, dtype=np.uint32) % GR]).astype(np.uint32)
    want = np.full((GR + body + GR, rb), P, np.uint8)
    G.gather_ref(want[GR:GR + body], miss_tab, n_miss, ms, md, 63)
    G.gather_ref(want[GR:GR + body], cache_tab, n_cache, cs, cd)
    out = torch.from_numpy(np.full_like(want, P)).cuda()
    miss_rows = torch.from_numpy(miss_tab).pin_memory() if host_rows else dev(miss_tab)
    kw = {}
    if counts == "device":
        kw["d_counts"] = dev(np.array([n_miss, n_cache], np.uint32))
    else:
        kw.update(num_miss=n_miss, num_cache=n_cache)
    lab = lab_want = None
    if label is not None:
        esz, num = label
        npt, tt = LABEL_TYPES[esz]
        lab_tab = rs.integers(0, 256, size=5000 * esz, dtype=np.uint8).view(npt)
        lab_idx = rs.integers(0, 5000, size=num).astype(np.uint32)
        lab_want = np.full((num + 16) * esz, P, np.uint8).view(npt)
        lab_want[8:8 + num] = lab_tab[lab_idx]
        lab = torch.from_numpy(np.full((num + 16) * esz, P, np.uint8)).cuda().view(tt)
        kw.update(label_out=lab[8:8 + num], label_src=torch.from_numpy(lab_tab.view(np.uint8)).cuda().view(tt),
                  label_index=dev(lab_idx))
    seg_dst = seg_want = None
    if num_segs:
        segs, d_words, s_words = _segments(rs, num_segs)
        seg_src_np = rs.integers(0, 1 << 32, size=s_words, dtype=np.uint64).astype(np.uint32)
        seg_want = np.full(d_words * 4, P, np.uint8).view(np.uint32)
        for d_at, s_at, w in segs:
            seg_want[d_at:d_at + w] = seg_src_np[s_at:s_at + w]
        seg_src = dev(seg_src_np)
        seg_dst = torch.from_numpy(np.full(d_words * 4, P, np.uint8)).cuda().view(torch.int32)
        kw["copies"] = [(hip.DevicePointer(seg_dst.data_ptr() + 4 * d_at), hip.DevicePointer(seg_src.data_ptr() + 4 * s_at),
                         w) for d_at, s_at, w in segs]
    lists = [dev(a) if len(a) else None for a in (ms, md, cs, cd)]
    grid, band = hip.extract_fused(out[GR:GR + body], miss_rows, dev(cache_tab), *lists, miss_row_mask=63,
                                   link_workgroups=link, **kw)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    if lab is not None:
        assert lab.cpu().numpy().tobytes() == lab_want.tobytes()
    if seg_dst is not None:
        assert host_u32(seg_dst).tobytes() == seg_want.tobytes()
    return grid, band


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
def test_fused_label_tail_element_sizes(hip, cus, esz):
    """the label rows riding on the extraction, every element size: a count that is no multiple of 256, and one beyond
    what the HBM band's workgroups take in one trip"""
    for k, num in enumerate((997, cus * G.VEC_WG_PER_CU * G.KBLOCK + 77)):
        grid, band = _run_fused(hip, 2, 50, 70, seed=40 + 2 * esz + k, label=(esz, num))
        assert band == 0 and grid == min(-(-num // G.KBLOCK), cus * G.VEC_WG_PER_CU)


FUSED_JOBS = {
    # chunks per row, misses, hits, counts, list capacity beyond the counts, link band asked for, miss rows in host memory
    "cpr1-32segments-link16": dict(cpr=1, n_miss=3001, n_cache=4099, link=16, host_rows=True, num_segs=G.MAX_COPY_SEGMENTS),
    "cpr25-device-0-k-hostrows-nolink": dict(cpr=25, n_miss=0, n_cache=2111, counts="device", pad=100, host_rows=True),
    "cpr32-device-k-0-hbm-nolink": dict(cpr=32, n_miss=1777, n_cache=0, counts="device", pad=100),
    "cpr64-band-wider-than-needed": dict(cpr=64, n_miss=10, n_cache=3000, link=64, host_rows=True),
    "cpr65-band-of-one": dict(cpr=65, n_miss=300, n_cache=1500, link=1, host_rows=True, label=(8, 333)),
    "cpr32-hostcounts-hbm-nolink": dict(cpr=32, n_miss=2500, n_cache=2500, num_segs=5, label=(4, 100)),
}


@pytest.mark.parametrize("name", list(FUSED_JOBS))
def test_fused_job_shapes(hip, name):
    job = FUSED_JOBS[name]
    grid, band = _run_fused(hip, seed=sorted(FUSED_JOBS).index(name), **job)
    link = job.get("link", 0)
    if link and job["n_miss"]:
        need = -(-job["n_miss"] * job["cpr"] // (G.KBLOCK * 4))
        assert band == min(link, need) and grid > band
        if name == "cpr64-band-wider-than-needed":
            assert band < link
        if name == "cpr65-band-of-one":
            assert band == 1
    else:
        assert band == 0 and grid > 0


def test_fused_refusals_launch_nothing_and_a_valid_job_is_planned(hip, cus):
    """refusals through fgnn_extract_fused_grid(job) == 0: nothing is launched, so counts may be as large as the window
    below 2^32 needs without any buffer of that size"""
    L = hip.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    grid_cap = cus * G.VEC_WG_PER_CU

    def job(**kw):
        j = hip.ExtractJob()
        j.out, j.miss_rows, j.cache_rows = base, base + 1024, base + 2048
        j.miss_src = j.miss_dst = j.cache_src = j.cache_dst = idx.data_ptr()
        j.num_miss, j.num_cache, j.dim, j.dtype, j.miss_row_mask = 4, 4, 16, hip.U8, 0xFFFFFFFF
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def grid(j):
        return int(L.fgnn_extract_fused_grid(C.byref(j)))

    segs = (hip.CopySegment * (G.MAX_COPY_SEGMENTS + 1))()
    for s in segs:
        s.dst, s.src, s.words = base, base + 2048, 4
    assert grid(job(segs=segs, num_segs=G.MAX_COPY_SEGMENTS)) > 0
    refused = {
        "out misaligned": job(out=base + 8),
        "miss rows misaligned": job(miss_rows=base + 1024 + 4),
        "cache rows misaligned": job(cache_rows=base + 2048 + 8),
        "one segment too many": job(segs=segs, num_segs=G.MAX_COPY_SEGMENTS + 1),
        "rows that are not whole chunks": job(dim=24),
        # the hit list's walk: total + grid * tile = 2^32 + 1
        "hit count in the window": job(num_cache=(1 << 32) - grid_cap * 1024 + 1),
        "miss count in the window (no link band)": job(num_miss=0xFFFFFC00),
        "miss count in the window (link band of 16)": job(num_miss=(1 << 32) - 16 * 1024 + 1, link_workgroups=16),
        "device counts with a capacity in the window": job(d_counts=idx.data_ptr(), cap=0xFFFFFFFE),
        "2^32 chunks": job(num_cache=1 << 32),
    }
    big = (hip.CopySegment * 2)()
    for s in big:
        s.dst, s.src, s.words = base, base + 2048, 1 << 30
    refused["copy words summing to 2^31"] = job(segs=big, num_segs=2)
    for why, j in refused.items():
        assert grid(j) == 0, why
        assert int(L.fgnn_extract_fused_link_grid(C.byref(j))) == 0, why
    # the largest counts the rule admits are planned (and not launched): total + grid * tile == 2^32
    assert grid(job(num_cache=(1 << 32) - grid_cap * 1024)) == grid_cap
    assert grid(job(num_miss=(1 << 32) - 16 * 1024, num_cache=0, link_workgroups=16)) == 16
    # afterwards a valid job still gets its grid
    assert grid(job()) == 1 and grid(job(num_cache=3000)) == 3


# ---- the batch driver with other feature and label types -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_graph():
    from fgnn_hip import synth
    return synth.powerlaw_csr(3000, 60000, seed=21)


@pytest.mark.parametrize("cached", [False, True], ids=["run_batch", "run_batch_cached"])
@pytest.mark.parametrize("dim,label", [(128, "I32"), (24, "U8"), (100, "I64")])
def test_batch_driver_with_f16_features_and_other_labels(hip, small_graph, dim, label, cached):
    """256-byte and 48-byte rows ride the chunk kernels with the labels in their tail; 200-byte rows take the element
    kernel and the labels a launch of their own.  feat() = feat_table[input_nodes()], label() = label_table[seeds]."""
    indptr, indices = small_graph
    num_node, batch, fanouts = 3000, 200, [5, 3]
    rs = np.random.default_rng(dim)
    feat = rs.standard_normal((num_node, dim)).astype(np.float16)
    npt = {"I32": np.int32, "U8": np.uint8, "I64": np.int64}[label]
    labels = rs.integers(0, 200, size=num_node).astype(npt)
    table, rank = G.cache_table(num_node, 0.25, seed=5)
    sampler = hip.Sampler(dev(indptr), dev(indices.copy()), fanouts, batch, sample_type=hip.KHOP2, seed=0x5A4D47)
    bt = sampler.new_batch(dim, hip.F16, getattr(hip, label))
    d_feat, d_label, d_table = dev(feat), dev(labels), dev(table)
    d_cache = dev(feat[rank[:num_node // 4]])
    for b in range(2):
        seeds = np.random.default_rng(b).permutation(num_node)[:batch if b == 0 else 31].astype(np.uint32)
        if cached:
            sampler.run_batch_cached(b, dev(seeds), 70 + b, bt, d_table, d_cache, d_feat, d_label)
        else:
            sampler.run_batch(b, dev(seeds), 70 + b, bt, d_table, d_feat, d_label)
        m = bt.wait()
        assert m.overflow == 0 and m.num_output == len(seeds) and m.num_miss + m.num_cache == m.num_input
        nodes = host_u32(bt.input_nodes())
        assert len(nodes) == m.num_input >= len(seeds) and (host_u32(bt.output_nodes()) == seeds).all()
        assert bt.feat().cpu().numpy().tobytes() == feat[nodes].tobytes()
        got = bt.label().cpu().numpy()
        assert got.dtype == npt and got.tobytes() == labels[seeds].tobytes()


# ---- the cache split around its items-per-thread switch ------------------------------------------------------------------------

SPLIT_NODES = 1 << 21


@pytest.fixture(scope="module")
def split_inputs():
    """node lists are drawn once (the longest, then prefixes) and the tables once per hit fraction"""
    nodes = np.random.default_rng(77).integers(0, SPLIT_NODES, size=(5 << 20) + 64).astype(np.uint32)
    return nodes, {f: G.cache_table(SPLIT_NODES, f, seed=3)[0] for f in (0.0, 1.0, 0.3)}


@pytest.mark.parametrize("frac", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("device_count", [False, True], ids=["host-count", "device-count"])
@pytest.mark.parametrize("n", [(4 << 20) - 1, 4 << 20, (4 << 20) + 1, (4 << 20) + 257, 5 << 20])
def test_cache_split_both_sides_of_the_items_per_thread_switch(hip, split_inputs, n, device_count, frac):
    """fgnn_get_miss_cache_index with a capacity of n nodes: one item per thread up to 4 << 20, eight beyond.  With a
    device-side count below the capacity the node list's tail holds valid ids, and what the kernel must not write
    (the lists beyond their counts, their guards) stays poisoned."""
    all_nodes, tables = split_inputs
    table = tables[frac]
    cap = n
    count = cap - 12345 if device_count else cap
    nodes = all_nodes[:cap]
    want = G.split_ref(table, nodes[:count])
    L = hip.load()
    d_nodes, d_table = dev(nodes), dev(table)
    outs = [torch.full((cap + 16,), -0x5A5A5A5B, dtype=torch.int32, device="cuda") for _ in range(4)]
    d_counts = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    d_n = dev(np.array([count], np.uint32)) if device_count else None
    ws = hip.scratch(cap, d_nodes.device)
    rc = L.fgnn_get_miss_cache_index(d_table.data_ptr(), d_nodes.data_ptr(), 0 if device_count else count,
                                     d_n.data_ptr() if device_count else None, cap, *[t.data_ptr() for t in outs],
                                     d_counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert d_counts.cpu().tolist() == [len(want[0]), len(want[2])] and len(want[0]) + len(want[2]) == count
    for got, w in zip(outs, want):
        got = host_u32(got)
        assert np.array_equal(got[:len(w)], w)
        assert (got[len(w):] == np.uint32(0xA5A5A5A5)).all()
