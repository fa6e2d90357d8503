"""The MX tests' own reference and checker (tests/mx_cases.py), on the CPU: the table-search e4m3 rounding against torch's
float8_e4m3fn, the vectorised rule against mx_quant_ref, that assert_mx_within tells a wrong code / a wrong scale byte from a
right one, and that the LayerNorm inputs of tests/test_mx_kernels_gpu.py respect the caps on ambiguous elements and blocks."""
import numpy as np
import pytest
import torch

import mx_cases as mc


def _torch_e4m3(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_rne_e4m3_equals_torch_float8_e4m3fn():
    rng = np.random.default_rng(0)
    mid = (mc.E4M3[:-1] + mc.E4M3[1:]) / 2                       # every tie: 9 significant bits at most, exact in fp32
    parts = [rng.uniform(-448, 448, 200_000), mid, -mid, mc.E4M3, -mc.E4M3, np.array([-0.0, 0.0]),
             np.linspace(-2.0 ** -6, 2.0 ** -6, 20_001),         # the subnormal codes and their neighbourhood
             np.nextafter(mid.astype(np.float32), np.float32(0)), np.nextafter(mid.astype(np.float32), np.float32(500))]
    for p in parts:
        x = np.asarray(p, np.float32)
        assert np.all(np.abs(x) <= 448)
        got, want = mc._rne_e4m3(x.astype(np.float64)), _torch_e4m3(x)
        assert np.array_equal(got, want), (x[got != want][:8], got[got != want][:8], want[got != want][:8])


def test_rule_byte_equals_mx_quant_ref_on_and_next_to_every_boundary():
    amax = []
    for X in (-127, -126, -60, -1, 0, 1, 37, 119):
        edge = np.float32(448.0 * 2.0 ** X)
        amax += [edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(np.inf)), edge * np.float32(0.6), edge / 2]
    amax += [np.float32(1e-45), np.float32(1e-42), np.float32(3e38), np.float32(1.0)]
    x = np.zeros((len(amax), 32), np.float32)
    x[:, 7] = amax
    _, s = mc.mx_quant_ref(x)
    assert np.array_equal(mc.rule_byte(np.asarray(amax, np.float64)), s[:, 0])
    assert mc.rule_byte(np.array([0.0]))[0] == 0


def test_admissible_bytes_and_codes_of_a_hand_made_block():
    y = np.zeros((1, 64))
    e = np.zeros((1, 64))
    y[0, 0], e[0, 0] = 448.0, 1.0                                # amax in [447, 449]: X = 0 or 1
    y[0, 1], e[0, 1] = 1.0 + 2.0 ** -4, 2.0 ** -10               # a tie of X = 0 (codes 0x38 | 0x39) inside the interval
    y[0, 2], e[0, 2] = -3.0, 0.0
    y[0, 40] = -0.0                                              # second block: all zero
    s_lo, s_hi, code_range = mc.admissible(y, e)
    assert (s_lo[0, 0], s_hi[0, 0]) == (127, 128) and (s_lo[0, 1], s_hi[0, 1]) == (0, 0)
    lo, hi = code_range(np.array([[127, 0]]))
    assert (lo[0, 1], hi[0, 1]) == (mc._key(0x38), mc._key(0x39))
    assert lo[0, 2] == hi[0, 2] == mc._key(mc._rne_e4m3(np.array(-3.0)))
    assert lo[0, 3] == hi[0, 3] == mc._key(0x00) and lo[0, 40] == hi[0, 40] == mc._key(0x00)
    lo, hi = code_range(np.array([[128, 0]]))
    assert lo[0, 2] == hi[0, 2] == mc._key(mc._rne_e4m3(np.array(-1.5)))
    assert mc._key(0x80) < mc._key(0x00) < mc._key(0x01) and mc._key(0x81) < mc._key(0x80)


def _encoded(rows, C):
    """a LayerNorm case with an encoding that is right: the fp64 reference rounded to fp32, then the rule"""
    _, _, _, ref, err = mc.ln_case(rows, C, True)
    q, s = mc.mx_quant_ref(ref.astype(np.float32))
    return q, s, ref, err


def test_checker_accepts_the_rule_and_a_non_finite_row():
    q, s, ref, err = _encoded(33, 288)
    blocks, elements = mc.assert_mx_within(q, s, ref, err, "rule")
    assert 0 <= blocks <= mc.CAP_BLOCKS and 0 <= elements <= mc.CAP_ELEMENTS
    ref = ref.copy()
    ref[4, 100] = np.nan
    q, s = q.copy(), s.copy()
    q[4, 96:128], s[4, 3] = 0x7F, 0xFF
    mc.assert_mx_within(q, s, ref, err, "NaN block")
    q[4, 97] = 0xFF
    with pytest.raises(AssertionError, match="element codes"):
        mc.assert_mx_within(q, s, ref, err, "NaN block with a negative NaN code")
    q[4, 97], s[4, 3] = 0x7F, 0xFE
    with pytest.raises(AssertionError, match="scale bytes"):
        mc.assert_mx_within(q, s, ref, err, "NaN block with a finite scale")


def test_checker_refuses_one_code_moved_by_one_at_an_unambiguous_element():
    q, s, ref, err = _encoded(33, 288)
    _, _, code_range = mc.admissible(ref, err)
    lo, hi = code_range(s)
    sure = np.argwhere((lo == hi) & ((q & 0x7F) > 0) & ((q & 0x7F) < 126))
    assert len(sure) > 0.9 * q.size
    for r, c in sure[[0, len(sure) // 2, -1]]:
        for step in (1, -1):
            bad = q.copy()
            bad[r, c] = int(q[r, c]) + step
            with pytest.raises(AssertionError, match="1 of .* element codes"):
                mc.assert_mx_within(bad, s, ref, err, "moved code")
    flipped = q.copy()
    flipped[sure[0][0], sure[0][1]] ^= 0x80
    with pytest.raises(AssertionError, match="element codes"):
        mc.assert_mx_within(flipped, s, ref, err, "flipped sign")


def test_checker_refuses_one_scale_byte_moved_by_one_at_an_unambiguous_block():
    q, s, ref, err = _encoded(33, 288)
    s_lo, s_hi, _ = mc.admissible(ref, err)
    sure = np.argwhere(s_lo == s_hi)
    assert len(sure) > 0.9 * s.size
    for r, j in sure[[0, len(sure) // 2, -1]]:
        for step in (1, -1):
            bad = s.copy()
            bad[r, j] = int(s[r, j]) + step
            with pytest.raises(AssertionError, match="1 of .* scale bytes"):
                mc.assert_mx_within(q, bad, ref, err, "moved scale")


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("rows,C", mc.LN_SHAPES)
def test_layernorm_inputs_respect_the_caps(rows, C, with_b):
    """The caps are conditions on the test input, established from the reference alone: with few ambiguous elements and blocks
    assert_mx_within demands bit equality nearly everywhere.  An input that exceeds a cap is changed, never the cap."""
    _, _, _, ref, err = mc.ln_case(rows, C, with_b)
    blocks, elements = mc.ambiguity(ref, err)
    print(f"layernorm_mx {rows} x {C} b={with_b}: {100 * elements:.2f} % of elements admit two codes, {100 * blocks:.2f} % of blocks two bytes")
    assert elements <= mc.CAP_ELEMENTS and blocks <= mc.CAP_BLOCKS, (elements, blocks)


def test_quant_inputs_hold_the_special_blocks():
    x = mc.quant_input(130, 224)
    blocks = x.reshape(-1, 32)
    assert np.any(np.all(blocks == 0, axis=1) & np.all(np.signbit(blocks), axis=1))          # all -0.0
    amax = np.abs(blocks).max(axis=1)
    for a in mc._MANT_AMAX:
        assert np.any(amax == a), a
    fin = np.all(np.isfinite(blocks), axis=1)
    assert (~fin).sum() == 3
    neg = blocks[fin][np.arange(fin.sum()), np.abs(blocks[fin]).argmax(axis=1)] < 0
    assert neg.any() and (~neg).any()
    for rows, K in mc.QUANT_SHAPES:
        assert mc.quant_input(rows, K).shape == (rows, K)
    assert [(r * k // 32) % 64 for r, k in mc.QUANT_SHAPES] == [1, 7, 9, 25, 14, 0]
