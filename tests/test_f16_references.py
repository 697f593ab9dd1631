"""CPU-only: the half-precision feature path exists at the kernel library's surface -- the three fp16-row entry points
in the built library, the header and the binding's signature table -- and the float64 numpy reference the GPU tests
hold them to (tests/f16_refs.py) agrees with train_refs.aggregate_ref applied to the upcast rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import f16_refs as F
import train_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fgnn_block_aggregate_ex_f16": "fgnn_block_aggregate_ex", "fgnn_block_aggregate_scaled_f16":
       "fgnn_block_aggregate_scaled", "fgnn_sage_finish_z_f16": "fgnn_sage_finish_z"}


def test_new_entry_points_are_exported_declared_and_typed_like_their_fp32_twins():
    from fgnn_hip import lib
    so = ctypes.CDLL(lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fgnn_hip.h")).read(), flags=re.S)
    L = lib.load()
    for name, twin in NEW.items():
        assert hasattr(so, name), name
        proto = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, header)
        assert proto and re.search(r"\bconst void \*h\b", proto.group(1)), name
        assert name in lib.EXPORTS and lib.SIGNATURES[name] == lib.SIGNATURES[twin], name
        assert tuple(getattr(L, name).argtypes) == lib.SIGNATURES[name][1] and getattr(L, name).restype is ctypes.c_int


def test_every_required_shape_is_among_the_cases():
    ex, sc = F.ex_cases(), F.scaled_cases()
    assert {c[1] for c in ex} == {c[1] for c in sc} == {1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 257, 600}
    assert {c[0] for c in ex} == {"e1", "e31", "e32", "e33", "e65", "hub_unsorted", "empty"}
    assert {c[2] for c in ex} == {True, False}
    assert {c[3] for c in sc} == set(F.MODE_PAIRS) and len(F.MODE_PAIRS) == 9
    for d in F.DIMS:  # an even and an odd stride above dim, an aligned and an odd base, at every dim
        lds = {(sum(F.H_FRAMES[c[2]]) + d) % 2 for c in sc if c[1] == d}
        bases = {F.H_FRAMES[c[2]][0] % 2 for c in sc if c[1] == d}
        assert lds == {0, 1} and bases == {0, 1}, d
    assert all(sum(f) > 0 for f in F.H_FRAMES)
    row, col = F.structure("hub_unsorted")[:2]
    assert row.numel() == 6600 and int(torch.bincount(col.long()).max()) >= 6001
    hub = (col == 137).nonzero().flatten()
    assert not bool((col[1:] >= col[:-1]).all()) and int(hub[-1] - hub[0]) >= 6500  # scattered, not one run
    assert [F.structure(s)[0].numel() for s in ("e1", "e31", "e32", "e33", "e65", "empty")] == [1, 31, 32, 33, 65, 0]


@pytest.mark.parametrize("case", [c for c in F.scaled_cases() if c[1] in (3, 64, 257)], ids=F.case_id)
def test_numpy_reference_agrees_with_train_refs_on_the_upcast_rows(case):
    name, dim, frame, (src_mode, dst_mode), weighted = case
    row, col, w, src_deg, dst_deg = F.structure(name)
    hbig, obig = F.tensors(dim, frame)
    h16 = F.h_of(hbig, dim, frame)
    out0 = obig[:, R.O_OFF:R.O_OFF + dim]
    kw = dict(w=w if weighted else None, num_dst=F.NDST, src_deg=src_deg if src_mode else None, src_mode=src_mode,
              dst_deg=dst_deg if dst_mode else None, dst_mode=dst_mode, out0=out0)
    ref, S, k = F.aggregate_ref_f16(row.numpy(), col.numpy(), h16=h16, **{a: (v.numpy() if isinstance(v, torch.Tensor)
                                                                             else v) for a, v in kw.items()})
    tref, tS, tk = R.aggregate_ref(row, col, h=h16.float(), **kw)
    assert np.array_equal(k, tk.numpy())
    # two float64 evaluations that differ in the order of the additions and in pow(-0.5) against 1 / sqrt: a few 2^-53
    # of the terms' magnitudes per edge
    tol = (k[:, None] + 8) * 2.0 ** -51 * S
    assert (np.abs(ref - tref.numpy()) <= tol).all() and (np.abs(S - tS.numpy()) <= tol).all()
    # the upcast the kernels make is the one numpy makes
    assert np.array_equal(h16.float().numpy().astype(np.float64), F.f16_to_f64(h16))
    assert torch.equal(F.bound(S, k), R.aggregate_bound(torch.from_numpy(S), torch.from_numpy(k)))


def test_test_rows_hold_subnormals_zeros_and_the_largest_half():
    hbig, _ = F.tensors(64, 0)
    a = np.abs(hbig.numpy().astype(np.float64))
    assert ((a > 0) & (a < 2.0 ** -14)).any() and (a == 0).any() and (a == 65504.0).any() and np.isfinite(a).all()
