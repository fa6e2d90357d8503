"""The tests of tests/test_wgrad_gpu.py's instrument, and backward.weight_grad's slicing rule -- on the CPU, no device.

  the table   wgrad_cases.slice_plan (written from the rule in include/m324.h and gemm.hip) reproduces the slice lengths that
              TN_CASES writes out as literals, never leaves a slice empty and stays inside the library's refusal rules;
  the power   every planted fault of wgrad_cases is caught by the checker the GPU tests call, at every case where it can occur
              (and every fault has such a case); the model without a fault passes everywhere;
  the caller  backward.weight_grad chooses `slices` from an occupancy target, the 2 GiB staging guard and the no-empty-slice rule:
              swept over the model's Linear shapes and token counts up to 2^22 with meta tensors (no memory) and a recording
              stand-in for ops.gemm_tn."""
import pytest
import torch

import wgrad_cases as wc
from conftest import CASES

BF = torch.bfloat16
IDS = [wc.case_id(c) for c in wc.TN_CASES]


# ------------------------------------------------------------------------------------------- the table and the slicing rule
@pytest.mark.parametrize("c", wc.TN_CASES, ids=IDS)
def test_slice_plan_reproduces_the_table(c):
    used, ks, lengths = wc.slice_plan(c.M, c.slices)
    assert tuple(lengths) == c.lengths and used == len(c.lengths) and sum(lengths) == c.M
    assert ks % 64 == 0 and all(n == ks for n in lengths[:-1]) and 0 < lengths[-1] <= ks
    assert wc.big_applies(c.M, c.N, c.Kc, used) == c.big                      # the kernel column of the table, by gemm.hip's rule
    assert c.N % 8 == 0 and c.Kc % 8 == 0 and c.N >= 8 and c.Kc >= 8


def test_the_table_has_what_the_gpu_tests_need():
    big = [c for c in wc.TN_CASES if c.big]
    assert sorted(c.lengths[-1] // 32 for c in big if len(c.lengths) > 1) == [1, 2, 3, 4, 8]      # the ring prologue run short: NH 1, 2
    assert {c.M for c in wc.TN_CASES} >= {1, 8, 63, 64, 65} and any(c.N == 8 for c in wc.TN_CASES) and any(c.Kc == 8 for c in wc.TN_CASES)
    assert any(c.lengths[-1] == 1 and len(c.lengths) > 1 for c in wc.TN_CASES)
    assert len(set(IDS)) == len(IDS)
    # one condition short of big, each condition once
    near = [c for c in wc.TN_CASES if not c.big and c.M >= 1296]
    assert [(c.M % 32 == 0, c.N % 256 == 0, c.M // len(c.lengths) >= 256) for c in near] == [(False, True, True), (True, False, True), (True, True, False)]


def test_slice_plan_over_every_small_m():
    """every M in 1 .. 4200 and every slices in 1 .. 70: the plan covers the tokens once, in whole 64-row tiles, leaves no slice
    empty, is accepted by the library's rules and is a fixed point of the clamp"""
    for M in range(1, 4201):
        for asked in range(1, 71):
            used, ks, lengths = wc.slice_plan(M, asked)
            assert 1 <= used <= asked and len(lengths) == used and sum(lengths) == M and min(lengths) > 0, (M, asked)
            assert ks == wc.tokens_per_slice(M, used) and ks % 64 == 0 and all(n == ks for n in lengths[:-1]) and lengths[-1] <= ks
            assert wc.accepted(M, used) and used <= -(-M // 64), (M, asked, used)
            assert wc.slice_plan(M, used)[0] == used
            # the clamp gives up no slice it could keep: every count between the one used and the one asked leaves a slice empty
            assert not any(wc.accepted(M, s) for s in range(used + 1, min(asked, -(-M // 64)) + 1)), (M, asked, used)
    assert not wc.accepted(65, 3) and wc.accepted(65, 2) and not wc.accepted(64, 0) and not wc.accepted(1 << 22, 65536) and not wc.accepted(0, 1)


# ------------------------------------------------------------------------------------------- the planted faults
def _layout(c, used, ldc_pad=4, col0=0, gap=3):
    return wc.Layout(c.N, c.Kc, used, c.Kc + ldc_pad, col0, gap)


def _operands(c, kind):
    return wc.int_operands(c.M, c.N, c.Kc, 7) if kind == "int" else wc.probe_operands(c.M, c.N, c.Kc)


@pytest.mark.parametrize("kind", ["int", "probe"])
@pytest.mark.parametrize("c", wc.TN_CASES, ids=IDS)
def test_the_model_without_a_fault_passes(c, kind):
    x, y = _operands(c, kind)
    used, _, lengths = wc.slice_plan(c.M, c.slices)
    parts = wc.emulate(x, y, c.slices)
    assert parts.shape == (used, c.N, c.Kc) and torch.equal(parts.float().double(), parts)         # integers below 2^24: exact in fp32
    assert float(parts.abs().max()) < 2 ** 24
    for lay in (_layout(c, used), wc.Layout(c.N, c.Kc, used, c.Kc + 64, 4, 0)):
        windows, whole = wc.c_buffer(lay)
        wc.emulate_into(whole, lay, x, y)
        wc.check_c(windows, whole, x, y, lengths, wc.case_id(c))
    wc.check_total(parts.sum(0).float(), x, y, wc.case_id(c))


@pytest.mark.parametrize("kind", ["int", "probe"])
@pytest.mark.parametrize("fault", wc.FAULTS)
def test_planted_fault_is_caught(fault, kind):
    """the checker fails for `fault` at EVERY case of the table where the fault can occur, and there is such a case.  The GPU tests
    run both kinds of operands at every case, so a fault has to be caught by one of them; the integer operands catch all, and the
    probe has ONE blind spot, pinned here: it repeats after lcm(256, 5) = 1280 tokens at N = 256 (X after N tokens, Y after 5), so
    at M = 1344 half-tile 1 of the first slice IS the half-tile it stands in for (tokens 1312 .. 1343 = 32 .. 63 + 1280)."""
    blind = {("short_ring_reads_slot_of_previous_slice", "probe", "1344x256x512s5")}
    hit = 0
    for c in wc.TN_CASES:
        used, _, lengths = wc.slice_plan(c.M, c.slices)
        lay = _layout(c, used)
        if not wc.fault_can_occur(fault, c, lay.ldc, lay.col0):
            continue
        hit += 1
        x, y = _operands(c, kind)
        windows, whole = wc.c_buffer(lay)
        wc.emulate_into(whole, lay, x, y, fault)
        if (fault, kind, wc.case_id(c)) in blind:
            wc.check_c(windows, whole, x, y, lengths, f"{fault} at {wc.case_id(c)}")
            continue
        with pytest.raises(AssertionError):
            wc.check_c(windows, whole, x, y, lengths, f"{fault} at {wc.case_id(c)}")
    assert hit > 0, f"no case of TN_CASES at which {fault} can occur"


def test_a_covered_gap_is_invisible_in_the_sum():
    """why the partials are looked at: a slice that begins one stage late, covered by the slice in front of it, leaves the sum right"""
    c = next(c for c in wc.TN_CASES if c.M == 200)
    x, y = wc.int_operands(c.M, c.N, c.Kc, 7)
    parts = wc.emulate(x, y, c.slices, "slice_begins_one_stage_late")
    wc.check_total(parts.sum(0).float(), x, y, "sum")
    assert not torch.equal(parts, wc.emulate(x, y, c.slices))


def test_operand_builders():
    x, y = wc.int_operands(200, 192, 328, 3)
    assert x.dtype == BF and y.dtype == BF and x.shape == (200, 192) and y.shape == (200, 328)
    assert float(x.float().abs().max()) == 8 and torch.equal(x.float(), x.float().round()) and torch.equal(x, wc.int_operands(200, 192, 328, 3)[0])
    x, y = wc.probe_operands(65, 264, 8)
    assert torch.equal(x.float().sum(1), torch.ones(65)) and float(x[5, 35]) == 1 and float(y[4, 5]) == (17 % 15) - 7
    a = wc.away_from_zero(300, 72, 5).float()
    assert float(a.abs().min()) >= 0.5 and float(a.abs().max()) <= 1.0 and bool((a < 0).any()) and bool((a > 0).any())


# ------------------------------------------------------------------------------------------- backward.weight_grad's slicing rule
def _linear_shapes():
    """(N, Ka) of the model's Linear layers as weight_grad sees them (both rounded up to the 64 the GEMM operands are padded to):
    the default architecture, the tiny test configuration, and one ragged pair"""
    from motion324_amd import synth
    shapes = set()
    for dims in (synth.Dims(), synth.Dims(**CASES["tiny"]["dims"])):
        for shape, kind in synth.state_dict_spec(dims).values():
            if kind.startswith("linear") or kind == "dino_qkv":
                n, ka = shape[0], int(torch.Size(shape[1:]).numel())
                shapes.add(((n + 63) // 64 * 64, (ka + 63) // 64 * 64))
    return sorted(shapes) + [(136, 72)]


M_SWEEP = list(range(1, 71)) + list(range(96, 2049, 32)) + [10368, 31104, 65536, 349440, 349504, 1 << 20, 1 << 22]


def _occupancy_target(M, N, Ka, big):
    """the slices weight_grad asks for before the guards: fill 256 CUs with 256 x 256 tiles (one 8-wave workgroup per CU, at most 64
    slices) or with 128 x 128 tiles (two workgroups per CU, at most 32), and at least 512 tokens per slice"""
    if big:
        return max(1, min(64, 252 // ((N // 256) * (Ka // 256)), M // 512))
    tiles = -(-N // 128) * -(-Ka // 128)
    return max(1, min(32, -(-640 // tiles), M // 512))


def _guards(M, slices, ld):
    while slices < 4096 and not wc.staging_ok(M, slices, ld):
        slices *= 2
    while slices > 1 and not wc.accepted(M, slices):
        slices -= 1
    return slices


def test_weight_grad_slicing_rule(monkeypatch):
    from motion324_amd import backward
    calls = []

    def record(x, y, slices=1, out=None, accumulate=False):
        calls.append((slices, out, accumulate))
        return out

    monkeypatch.setattr(backward.ops, "gemm_tn", record)
    shapes = _linear_shapes()
    assert (768, 768) in shapes and (2304, 768) in shapes and (768, 3072) in shapes and (192, 192) in shapes and len(shapes) >= 8
    marker = torch.empty((1,), device="meta")
    n_calls = n_big = n_doubled = 0
    for N, Ka in shapes:
        for M in M_SWEEP:
            for ldx, ldy in ((N, Ka), (N + 8, Ka + 8), (max(N, 3 * 768), Ka), (N, 4 * 3072), (4 * 3072, 4 * 3072)):
                dy = torch.empty((M, ldx), dtype=BF, device="meta")[:, :N]
                a = torch.empty((M, ldy), dtype=BF, device="meta")[:, ldy - Ka:]
                del calls[:]
                got = backward.weight_grad(dy, a, out=marker, accumulate=bool(M & 1))
                assert len(calls) == 1 and got is marker and calls[0][1] is marker and calls[0][2] == bool(M & 1)
                s = calls[0][0]
                what = (M, N, Ka, ldx, ldy, s)
                ld = max(ldx, ldy)
                assert 1 <= s <= 65535, what
                assert wc.accepted(M, s), what                                        # no empty slice
                assert wc.staging_ok(M, s, ld), what                                  # (ks + 64) * ld * 2 < 0x7FFFFFFF
                assert wc.slice_plan(M, s)[0] == s, what                              # ops.gemm_tn's clamp leaves it alone
                # the branch: the slices are those of the kernel the library will run with them
                big = wc.big_applies(M, N, Ka, s)
                assert s == _guards(M, _occupancy_target(M, N, Ka, big), ld), what + (big,)
                if M % 32 == 0 and N % 256 == 0 and Ka % 256 == 0 and M >= 512:
                    assert big, what                                                   # 512 tokens per slice at least: M / slices >= 256
                n_calls += 1
                n_big += big
                n_doubled += s > _occupancy_target(M, N, Ka, big)
    assert n_calls == len(shapes) * len(M_SWEEP) * 5 and n_big > 0 and n_doubled > 0 and n_big < n_calls


def test_weight_grad_sweep_reaches_both_sides_of_the_staging_guard():
    """the two token counts of the GPU test at ld = 3072, one slice: accepted, refused"""
    assert wc.staging_ok(349440, 1, 3072) and (349440 + 64) * 3072 * 2 == 2147352576
    assert not wc.staging_ok(349504, 1, 3072) and wc.tokens_per_slice(349504, 1) == 349504
    assert wc.big_applies(349440, 256, 256, 1) and not wc.big_applies(349440, 8, 8, 1)
