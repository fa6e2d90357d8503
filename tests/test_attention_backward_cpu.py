"""The inputs of tests/test_attention_backward_gpu.py would expose a backward kernel that is wrong at a tile, wave or workgroup edge --
shown without a GPU, on the CPU model of the kernels (attn_bwd_cases.model_kernel).

For every case of attn_bwd_cases.CASES: the model with the kernels' roundings lies within error_bounds.attention_backward of fp64
autograd (worst err / bound < 1, the gate of the GPU test), and every planted mistake the shape allows puts at least one of
dQ / dK / dV at 2 or more times its bound.  Both gates are conditions on the INPUTS: a mistake that is not detected means the
inputs must change, not the gate.  Ratios seen: tests/ERROR_BOUNDS.md.
"""
import pytest

import attn_bwd_cases as ac

NAMES = list(ac.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_edge_queries_have_two_dominant_keys_and_every_edge_key_is_one(name):
    """edge_inputs asserts it while it builds; here again from the finished operands, with the figures printed.  Score range below
    60 in the log2 domain: the same inputs are legal for the bounded-scores forward."""
    inp = ac.inputs(name)
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    top, lo, hi = ac.check_edge_structure(inp)
    print(f"[inputs] {name}: max |log2 score| {top:.1f}, pair probabilities {lo:.3f} .. {hi:.3f}, "
          f"{len(inp['eq'])} edge queries, {len(inp['ek'])} edge keys")
    assert top < ac.SCORE_RANGE
    if ac.degenerate(Lq, Lk):
        return
    assert set(inp["pairs"]) == set(ac.edge_queries(Lq)) and Lq - 1 in inp["pairs"] and 0 in inp["pairs"]
    assert {k for p in inp["pairs"].values() for k in p} == set(ac.edge_keys(Lk)) and Lk - 1 in ac.edge_keys(Lk)
    assert 0.2 <= lo <= hi <= 0.8


@pytest.mark.parametrize("name", NAMES)
def test_model_kernel_is_within_the_bound(name):
    got = ac.model_kernel(ac.inputs(name))
    r = ac.ratios(got, name)
    print(f"[model] {name}: worst err / bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v < 1.0 for v in r.values()), r


@pytest.mark.parametrize("name", NAMES)
def test_every_planted_mistake_is_far_outside_the_bound(name):
    inp = ac.inputs(name)
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    todo = ac.mistakes(inp)
    if not ac.degenerate(Lq, Lk):
        labels = [l for l, _ in todo]
        assert len([l for l in labels if l.startswith("drop key")]) == len(ac.edge_keys(Lk))
        assert len([l for l in labels if l.startswith("drop query")]) == len(ac.edge_queries(Lq))
        assert "dK without ln 2" in labels and "LSE of the next query" in labels
    missed, smallest = [], None
    for label, kw in todo:
        r = ac.ratios(ac.model_kernel(inp, **kw), name, keys=("dQ", "dK", "dV"))
        worst = max(r.values())
        print(f"[mistake] {name}: {label}: dQ {r['dQ']:.3g} dK {r['dK']:.3g} dV {r['dV']:.3g}")
        smallest = worst if smallest is None else min(smallest, worst)
        if not worst >= 2.0:
            missed.append((label, r))
    if todo:
        print(f"[mistake] {name}: smallest detection ratio {smallest:.3g} over {len(todo)} mistakes")
    assert not missed, missed
