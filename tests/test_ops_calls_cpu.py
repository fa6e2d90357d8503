"""motion324_amd.ops, the marshalling layer, checked without a device: every wrapper runs on small CPU tensors with libm324, the
stream and the device test replaced by recorders (tests/golden/make_ops_calls.py), and the C-ABI calls it makes -- entry points,
argument order, pointers and offsets, leading dimensions, flag words, the GemmArgs fields -- its span rows, the tensors it marks
as written, what it returns and the texts of its refusals must equal tests/golden/ops_calls.json.  That fixture was recorded from
the parent of the commit that gave ops.py one launch helper, one q|k|v-heads parser and a gemm() split by mode; its only patched
entries are the written-marks gemm(qkv_heads=...) gained then (make_ops_calls.EXPECTED)."""
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_ops_calls as calls      # noqa: E402

from motion324_amd import lib, ops      # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ops_calls.json")) as f:
        want = json.load(f)
    return want, calls.record(ops, lib)


def test_same_cases(recorded):
    want, got = recorded
    assert list(got) == list(want), "make_ops_calls.py enumerates other cases than ops_calls.json records"
    assert len(got) > 100


@pytest.mark.parametrize("name", [name for name, _ in calls.CASES])
def test_wrapper_marshals_as_recorded(recorded, name):
    want, got = recorded
    w, g = want[name], got[name]
    assert [c[0] for c in g["calls"]] == [c[0] for c in w["calls"]]
    for gc, wc in zip(g["calls"], w["calls"]):
        assert gc == wc
    assert g == w


def test_recorders_are_gone():
    with pytest.raises(lib.M324Error, match="HIP device tensors"):
        ops._p(torch.zeros(1))
    assert ops._stream.__module__ == ops.__name__ and ops.span.__module__ == "motion324_amd.timing"


def _heads(L, vshape):
    bf = torch.bfloat16
    return (None, torch.zeros((1, 1, L, 64), dtype=bf), torch.zeros(vshape, dtype=bf), None, None, 1e-5, 1.0, L, 1)


def test_gemm_mx_shares_gemms_heads_parser(monkeypatch):
    """the two things gemm_mx gained from the shared parser: the explicit tenth entry, and the refusal of a transposed V whose
    length is no multiple of 64 (which the kernel's 64-key groups cannot store)"""
    seen = []

    class Lib:
        def m324_gemm_mx(self, args, *rest):
            seen.append(args._obj.aux_mode)
            return 0
    monkeypatch.setattr(lib, "load", lambda: Lib())
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    a, w = ops.mx_empty(64, 64, "cpu"), ops.mx_empty(128, 64, "cpu")
    ops.gemm_mx(a, w, None, qkv_heads=_heads(64, (1, 1, 64, 64)))
    ops.gemm_mx(a, w, None, qkv_heads=_heads(64, (1, 1, 64, 64)) + (True,))
    ops.gemm_mx(a, w, None, qkv_heads=ops.QKVHeads(*_heads(64, (1, 1, 64, 64)), vt=True))
    assert seen == [3, 4, 4]                                        # M324_AUX_QKV_HEADS, then M324_AUX_QKV_HEADS_VT twice
    a40 = ops.mx_empty(40, 64, "cpu")
    with pytest.raises(lib.M324Error, match=r"gemm_mx: a transposed V output needs L % 64 == 0 \(L=40\)"):
        ops.gemm_mx(a40, w, None, qkv_heads=_heads(40, (1, 1, 64, 40)))
    assert len(seen) == 3


def test_qkvheads_is_the_tuple_it_replaces():
    t = _heads(64, (1, 1, 64, 64))
    h = ops.QKVHeads(*t)
    assert len(h) == 10 and all(x is y for x, y in zip(h, t + (None,))) and ops.QKVHeads(*t, True).vt is True
    assert ops.QKVHeads._fields == ("Q", "K", "V", "q_w", "k_w", "eps", "q_scale", "L", "H", "vt")
