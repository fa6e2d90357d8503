"""The optimizer step's kernels element by element against fp64 (bounds: tests/error_bounds.py, derivations: tests/ERROR_BOUNDS.md,
"The optimizer step"): m324_adamw, m324_adamw_flat, optim.FusedAdamW.step() as a whole, m324_weight_mirror from a hand-built table,
m324_grad_sumsq, m324_mse and m324_mse_bwd at their edges.  References are fp64 torch / numpy on the CPU, computed from the
operands the kernels read: the fp32 tensors and the fp32 values of the scalars.  Every worst err / bound is printed (run with -s):
the figures are records, the gate is 1.0."""
import math

import numpy as np
import pytest
import torch

import error_bounds as eb
import optimizer_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = eb.U32
WD = oc.HYPER["weight_decay"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _scalar(gs):
    return None if gs is None else torch.tensor(gs, dtype=torch.float32, device=DEV)


def _t(x):
    return torch.tensor(x, dtype=torch.float64)                  # (torch.tensor of a Python float is fp32: it would round the reference)


def _record(what, ratios):
    print(f"[worst err / bound] {what}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ------------------------------------------------------------------------------------------- 2. m324_adamw, m324_adamw_flat
def _launch(kind, ins, step, gs, n_decay=0, wd=WD, views=None):
    """One update by the kernel on device copies of ins = (p, g, m, v) (or in place on `views`); returns the CPU results."""
    from motion324_amd import ops
    d = [t.to(DEV) for t in ins] if views is None else views
    hp = oc.HYPER
    if kind == "flat":
        ops.adamw_flat(d[0], d[1], d[2], d[3], n_decay, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, step, _scalar(gs))
    else:
        ops.adamw_step(d[0], d[1], d[2], d[3], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, step, _scalar(gs))
    return d[0].cpu(), d[2].cpu(), d[3].cpu()


def _check(outs, ins, wd, step, gs, what, worst=None):
    """p', m' and v' each inside the bound of the fp64 update of `ins`; wd: scalar or per-element decay"""
    hp = dict(oc.HYPER, weight_decay=wd, step=step, grad_scale=None if gs is None else eb.f32(gs))
    refs, bounds = eb.adamw_reference(*ins, **hp), eb.adamw_step(*ins, **hp)
    ratios = {k: eb.assert_within(o, r, b, f"{what}: {k}") for k, o, r, b in zip(("p'", "m'", "v'"), outs, refs, bounds)}
    if worst is not None:
        for k, x in ratios.items():
            worst[k] = max(worst.get(k, 0.0), x)
    return refs, bounds


@pytest.mark.parametrize("step", oc.STEPS)
def test_adamw_flat_against_fp64(step):
    """n = 4 and 8 (one and two 16-byte units) with every n_decay, and 4096 + 4 with n_decay inside a workgroup's range"""
    worst = {}
    for gs in oc.GRAD_SCALES:
        for n, n_decay in ((4, 0), (4, 4), (8, 0), (8, 4), (8, 8), (4096 + 4, 2052)):
            ins = oc.adamw_inputs(n, step, seed=1000 + n)
            outs = _launch("flat", ins, step, gs, n_decay)
            _check(outs, ins, oc.decay_vector(n, n_decay, WD), step, gs, f"adamw_flat n {n} n_decay {n_decay} step {step} gs {gs}", worst)
    _record(f"adamw_flat step {step}", worst)


@pytest.mark.parametrize("step", oc.STEPS)
def test_adamw_step_against_fp64(step):
    worst = {}
    for gs in oc.GRAD_SCALES:
        for n in (1, 255):
            ins = oc.adamw_inputs(n, step, seed=2000 + n)
            _check(_launch("step", ins, step, gs), ins, WD, step, gs, f"adamw_step n {n} step {step} gs {gs}", worst)
    _record(f"adamw_step step {step}", worst)


def test_adamw_flat_grid_stride_loop_and_decay_boundary_in_the_wrapped_part():
    """n / 4 > 4096 * 256 units: the workgroups go round a second time (grid_for caps the grid at 4096), and n_decay lies in the
    units of that second round"""
    n4 = 4096 * 256 + 777
    n, n_decay = 4 * n4, 4 * (4096 * 256 + 300)
    worst = {}
    for step, gs in ((1, None), (3, 0.37), (20000, 1e-3)):
        ins = oc.adamw_inputs(n, step, seed=31)
        outs = _launch("flat", ins, step, gs, n_decay)
        _check(outs, ins, oc.decay_vector(n, n_decay, WD), step, gs, f"adamw_flat n {n} step {step}", worst)
    _record(f"adamw_flat n {n}", worst)


def test_adamw_step_grid_stride_loop_on_an_unaligned_view():
    """n > 4096 * 256 elements on views that start 4 bytes past a 16-byte boundary"""
    n = 4096 * 256 + 3 * 256 + 5
    views = [torch.zeros(n + 1, device=DEV)[1:] for _ in range(4)]
    assert all(vw.data_ptr() % 16 == 4 for vw in views)
    worst = {}
    for step, gs in ((2, 1e-3), (20000, None)):
        ins = oc.adamw_inputs(n, step, seed=32)
        for vw, t in zip(views, ins):
            vw.copy_(t)
        _check(_launch("step", ins, step, gs, views=views), ins, WD, step, gs, f"adamw_step n {n} step {step}", worst)
    _record(f"adamw_step n {n}", worst)


def test_adamw_flat_decay_boundary_discriminates():
    """The elements just before and just after n_decay are inside the bound, and at both the update with decay and the one without
    differ by far more than the bound: a boundary one unit off could not pass."""
    n, n_decay = 4096 + 4, 2052
    for step in (1, 100):
        p, g, m, v = oc.adamw_inputs(n, step, seed=41)
        p[n_decay - 4:n_decay + 4] = torch.tensor([0.7, -0.9, 1.1, -1.3, 1.4, -1.2, 0.8, -1.0])
        ins = (p, g, m, v)
        outs = _launch("flat", ins, step, 0.37, n_decay)
        refs, bounds = _check(outs, ins, oc.decay_vector(n, n_decay, WD), step, 0.37, f"boundary step {step}")
        swapped = eb.f32(WD) - oc.decay_vector(n, n_decay, WD)     # decay where there is none, none where there is
        other = eb.adamw_reference(*ins, **dict(oc.HYPER, weight_decay=swapped, step=step, grad_scale=eb.f32(0.37)))
        edge = slice(n_decay - 4, n_decay + 4)
        assert bool(((refs[0] - other[0]).abs()[edge] > 20 * bounds[0][edge]).all())
        assert not eb.violations(outs[0][edge], refs[0][edge], bounds[0][edge]).any()
        assert bool(eb.violations(outs[0][edge], other[0][edge], bounds[0][edge]).all())


@pytest.mark.parametrize("kind", ["flat", "step"])
def test_adamw_three_steps_on_the_kernels_own_state(kind):
    """three updates in a row, m and v (and p) fed back; each checked against the fp64 update of the state the kernel started
    that step from, so an error of one step is judged once and does not widen the next check"""
    n, n_decay = 4096 + 4, 2052
    p, g, m, v = oc.adamw_inputs(n, 1, seed=51)
    wd = oc.decay_vector(n, n_decay, WD) if kind == "flat" else WD
    worst = {}
    for step in (1, 2, 3):
        g = oc.adamw_inputs(n, 1, seed=51 + step)[1]
        outs = _launch(kind, (p, g, m, v), step, 0.37, n_decay)
        _check(outs, (p, g, m, v), wd, step, 0.37, f"adamw_{kind} chained step {step}", worst)
        p, m, v = outs
    _record(f"adamw_{kind} chained", worst)


def test_adamw_step_without_decay_equals_flat_without_decay_group():
    """weight_decay = 0 through m324_adamw and n_decay = 0 through m324_adamw_flat: the same update, each inside the one bound
    (not bit for bit: one divides by bc2_sqrt, the other multiplies by the reciprocal)"""
    n = 4096 + 4
    for step in (1, 100):
        ins = oc.adamw_inputs(n, step, seed=61)
        a = _launch("step", ins, step, 0.37, wd=0.0)
        b = _launch("flat", ins, step, 0.37, n_decay=0)
        refs, bounds = _check(a, ins, 0.0, step, 0.37, "adamw_step wd 0")
        _check(b, ins, oc.decay_vector(n, 0, WD), step, 0.37, "adamw_flat n_decay 0")
        for x, y, bd in zip(a, b, bounds):
            assert bool(((x.double() - y.double()).abs() <= 2 * bd).all())


# ------------------------------------------------------------------------------------------- 3. FusedAdamW.step()
CLIP, FACTOR = 1.0, 5.0
PARAM_SHAPES = [("b0", (1,), False), ("w0", (3, 768), False), ("e0", (8, 8), True), ("b1", (3,), False), ("w1", (130, 192), False),
                ("t0", (1, 5), False), ("b2", (4097,), False)]          # 1, 2304, 64, 3, 24960, 5 and 4097 elements


def _make_optimizer(flatten):
    from motion324_amd import optim
    named = []
    for i, (name, shape, no_decay) in enumerate(PARAM_SHAPES):
        gen = torch.Generator().manual_seed(300 + i)
        p = torch.nn.Parameter((torch.randn(shape, generator=gen) * (1.0 if len(shape) == 1 else 0.05)).to(DEV))
        if no_decay:
            p._no_weight_decay = True
        named.append((name, p))
    # a layout order that is NOT named_parameters() order: the checkpoint numbering has to undo it
    opt = optim.FusedAdamW(named, lr=oc.HYPER["lr"], betas=(oc.HYPER["beta1"], oc.HYPER["beta2"]), eps=oc.HYPER["eps"],
                           weight_decay=WD, grad_clip_norm=CLIP, allowed_gradnorm_factor=FACTOR, order=[p for _, p in reversed(named)],
                           flatten=flatten)
    return opt, dict(named)


def _padding_mask(opt):
    used = torch.zeros(opt.numel, dtype=torch.bool)
    for o, p in zip(opt.offsets, opt.params):
        used[o:o + p.numel()] = True
    return ~used


def _write_grads(opt, scale, seed, plant=None):
    """gradients straight into grad_of(p); plant: {name: [(flat index, value)]}.  Returns the CPU copies by layout slot."""
    grads = []
    for i, p in enumerate(opt.params):
        g = torch.randn(p.shape, generator=torch.Generator().manual_seed(seed + i)) * scale
        for idx, val in (plant or {}).get(opt.names[i], []):
            g.view(-1)[idx] = val
        opt.grad_of(p).copy_(g.to(DEV))
        grads.append(g)
    return grads


def _state(opt):
    return [t.clone() for t in (opt.flat_param, opt.m, opt.v)] + [[p.data.clone() for p in opt.params]]


@pytest.mark.parametrize("flatten", [True, False])
def test_fused_adamw_step_against_the_fp64_sequence(flatten):
    """nan_to_num(0, 1e-6, -1e-6) -> global L2 norm -> clip coefficient min(1, clip / (norm + 1e-6)) -> skip rule -> AdamW with decay
    on the decay group only (optim.py's docstring), on synthetic parameters with gradients written straight into the flat buffer.
    The reference update takes the coefficient the optimizer wrote (_gscale), which is itself checked against the fp64 norm."""
    opt, named = _make_optimizer(flatten)
    pad = _padding_mask(opt)
    assert int(pad.sum()) == 3 + 3 + 1 + 3 and opt.n_decay % 4 == 0 and opt.numel % 4 == 0
    assert [opt.names[i] for i in range(opt.n_decay_params)] == ["t0", "w1", "w0"] and opt.names[3:] == ["b2", "b1", "e0", "b0"]
    buffers = lambda: (opt.flat_param, opt.flat_grad, opt.m, opt.v)
    assert all(float(t.cpu()[pad].abs().max()) == 0.0 for t in buffers())
    inf, nan = float("inf"), float("nan")
    cases = [("below the clip", 0.002, None, True, False),
             ("above the clip", 0.02, None, True, False),
             ("non-finite gradients", 0.002, {"w1": [(0, nan), (24959, inf), (7777, -inf)], "b2": [(4096, nan), (1, -inf), (2, inf)],
                                               "e0": [(63, inf)], "b0": [(0, nan)]}, True, False),
             ("norm above factor * clip", 0.1, None, True, True),
             ("loss not finite", 0.002, None, False, True),
             ("after the skipped steps", 0.02, None, True, False)]
    worst, steps_done = {}, 0
    for k, (what, scale, plant, finite, want_skip) in enumerate(cases):
        grads = _write_grads(opt, scale, 400 + 10 * k, plant)
        before = _state(opt)
        info = opt.step(loss_is_finite=finite)
        clean = [torch.nan_to_num(g, nan=0.0, posinf=1e-6, neginf=-1e-6) for g in grads]
        fg = opt.flat_grad.cpu()
        for o, g in zip(opt.offsets, clean):                      # sanitised in place, bit for bit: 0 and +-1e-6 where planted
            assert torch.equal(_bits(fg[o:o + g.numel()]), _bits(g.reshape(-1))), what
        assert float(fg[pad].abs().max()) == 0.0
        # the norm and the coefficient
        total = float(sum((g.double() ** 2).sum() for g in clean))
        _, _, depth = eb.grad_sumsq_plan(opt.numel, opt.flat_grad.data_ptr() % 16 == 0)
        b_sum = eb.sum_of_squares(total, opt.numel, depth)
        worst["sum"] = max(worst.get("sum", 0.0), eb.assert_within(opt._sumsq, _t(total), _t(b_sum), what + ": sum of squares"))
        norm = math.sqrt(total)
        # optim.py, FusedAdamW.step: norm = float(_sumsq.sqrt()) -- |sqrt a - sqrt b| <= |a - b| / sqrt b on the sum's own bound, then ONE
        # fp32 sqrtf on the device (1 ulp: 2 U); coef = min(1, clip / (norm + 1e-6)) in host fp64 (no rounding counted), whose
        # error is coef e_norm / (norm + 1e-6 - e_norm) <= coef e_norm / (norm - e_norm); _gscale.fill_ rounds it to fp32 once: U coef
        e_norm = b_sum / norm + 2 * U * (norm + b_sum / norm)
        assert abs(info["grad_norm"] - norm) <= e_norm, what
        assert info["skipped"] == want_skip == ((not finite) or norm > FACTOR * CLIP), what
        if want_skip:                                             # nothing moved: bit-identical state, the step count stands
            after = _state(opt)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(after[:3], before[:3])), what
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(after[3], before[3])), what
            assert opt.step_count == steps_done
            continue
        steps_done += 1
        assert opt.step_count == steps_done
        coef = min(1.0, CLIP / (norm + 1e-6))
        got = float(opt._gscale)
        if norm + e_norm < CLIP - 1e-6:
            assert got == 1.0, what
        else:
            assert norm - e_norm > CLIP and abs(got - coef) <= coef * e_norm / (norm - e_norm) + U * coef, (what, got, coef)
        # the update, per parameter, from the state the optimizer held before the step
        for i, p in enumerate(opt.params):
            o, n = opt.offsets[i], p.numel()
            ins = (before[3][i].reshape(-1).cpu(), clean[i].reshape(-1), before[1][o:o + n].cpu(), before[2][o:o + n].cpu())
            outs = (p.data.reshape(-1).cpu(), opt.m[o:o + n].cpu(), opt.v[o:o + n].cpu())
            _check(outs, ins, WD if opt.decay[i] else 0.0, steps_done, got, f"{what}: {opt.names[i]}", worst)
            if flatten:
                assert p.data.data_ptr() == opt.flat_param.data_ptr() + 4 * o and torch.equal(p.data.reshape(-1), opt.flat_param[o:o + n])
            else:
                assert torch.equal(_bits(opt.flat_param[o:o + n]), _bits(before[0][o:o + n]))      # the parameters live elsewhere
        assert all(float(t.cpu()[pad].abs().max()) == 0.0 for t in buffers()), what
    assert steps_done == 4
    _record(f"FusedAdamW flatten={flatten}", worst)
    # the checkpoint carries the checked moments under the reference's numbering: named order, the decay group first
    sd = opt.state_dict()
    numbering = ["w0", "w1", "t0", "b0", "e0", "b1", "b2"]
    assert sd["param_names"] == numbering and sd["param_groups"][0]["params"] == [0, 1, 2]
    for k, name in enumerate(numbering):
        i = opt.names.index(name)
        o, n = opt.offsets[i], opt.params[i].numel()
        st = sd["state"][k]
        assert float(st["step"]) == 4.0 and st["exp_avg"].shape == named[name].shape
        assert torch.equal(_bits(st["exp_avg"].reshape(-1)), _bits(opt.m[o:o + n]))
        assert torch.equal(_bits(st["exp_avg_sq"].reshape(-1)), _bits(opt.v[o:o + n]))


# ------------------------------------------------------------------------------------------- 4. m324_weight_mirror
SENTINEL = 0x5A5A
MIRROR_SHAPES = [(1, 64), (3, 64), (64, 64), (65, 128), (130, 192), (2304, 768)]
SKIPPED, WIDE, ADVERSARIAL = 3, 1, 4              # the item without a transposed copy, the one with ldT 64 wider, the one with the values below
SPECIAL_BITS = [
    0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,            # ties over an even and an odd upper half, +-1 ulp
    0xBF808000, 0xBF818000, 0xBF807FFF, 0xBF808001, 0xBF817FFF, 0xBF818001,
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,    # +-0, +-inf, the largest finite values -> inf
    0x7FC00000, 0x7F800001, 0xFFC00001, 0x7F80FFFF,                                        # NaNs, two with the payload in the low half only
    0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007FFFFF,    # subnormals: ties, and one that rounds to a normal
    0x80000001, 0x80008001, 0x80400000, 0x807FFFFF]


def _mirror_case():
    from motion324_amd import lib
    specials = torch.from_numpy(np.array(SPECIAL_BITS, dtype=np.uint32).view(np.float32).copy())
    items, so, do, dto, tiles = [], 4, 8, 2, 0
    for j, (rows, cols) in enumerate(MIRROR_SHAPES):
        ldt = (rows + 63) // 64 * 64 + (64 if j == WIDE else 0)
        items.append(dict(rows=rows, cols=cols, ldT=ldt, src_off=so, dst_off=do, dstT_off=-1 if j == SKIPPED else dto, first_tile=tiles))
        so += rows * cols + 4 * (j + 1)                            # gaps between the items everywhere, of different widths
        do += rows * cols + 4 * (j + 2)
        dto += 0 if j == SKIPPED else cols * ldt + 2 * (j + 1)
        tiles += ((rows + 63) // 64) * (cols // 64)
    src = torch.full((so,), float("nan"))
    for j, it in enumerate(items):
        x = torch.randn(it["rows"] * it["cols"], generator=torch.Generator().manual_seed(500 + j))
        if j == ADVERSARIAL:
            x[:specials.numel()] = specials                        # the first row ...
            x[-specials.numel():] = specials                       # ... and the last, in the tile row that is only partly there
            x[64 * it["cols"] - 5:64 * it["cols"] - 5 + specials.numel()] = specials
        src[it["src_off"]:it["src_off"] + x.numel()] = x
    arr = (lib.MirrorItem * len(items))()
    for a, it in zip(arr, items):
        a.src_off, a.dst_off, a.dstT_off, a.first_tile = it["src_off"], it["dst_off"], it["dstT_off"], it["first_tile"]
        a.rows, a.cols, a.ldT = it["rows"], it["cols"], it["ldT"]
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    return items, src, table, tiles, do, dto


def _matches_torch_rounding(got, x):
    """got: int16 bit patterns of the kernel's bf16 values, x: the fp32 values they were made from.  The contract of
    include/m324.h, m324_weight_mirror: "Round to nearest even, as torch's .to(bfloat16)" -- torch's bit pattern for every input,
    fp32 subnormals and their ties included; a NaN stays a NaN (its payload is not compared).  Returns the mask of the elements
    that comply."""
    want = x.to(torch.bfloat16).view(torch.int16)
    return torch.where(torch.isnan(x), torch.isnan(got.view(torch.bfloat16).float()), got == want)


def test_weight_mirror_from_a_hand_built_table():
    from motion324_amd import ops
    items, src, table, tiles, n_dst, n_dstT = _mirror_case()
    assert tiles == 1 + 1 + 1 + 4 + 9 + 36 * 12
    sent = lambda n: torch.full((n,), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    src_d = src.to(DEV)
    for zeroed in (False, True):
        dst = sent(n_dst)
        dstT = torch.zeros(n_dstT, dtype=torch.bfloat16, device=DEV) if zeroed else sent(n_dstT)
        ops.weight_mirror(src_d, dst, dstT, table, len(items), tiles)
        assert torch.equal(_bits(src_d), _bits(src))               # the source is read only
        got, gotT = _bits(dst), _bits(dstT)
        fill = 0 if zeroed else SENTINEL
        seen, seenT = torch.zeros(n_dst, dtype=torch.bool), torch.zeros(n_dstT, dtype=torch.bool)
        for j, it in enumerate(items):
            rows, cols, ldt = it["rows"], it["cols"], it["ldT"]
            x = src[it["src_off"]:it["src_off"] + rows * cols].view(rows, cols)
            blk = got[it["dst_off"]:it["dst_off"] + rows * cols].view(rows, cols)
            ok = _matches_torch_rounding(blk, x)
            assert bool(ok.all()), (j, "row-major", ok.logical_not().nonzero()[:8].tolist())
            seen[it["dst_off"]:it["dst_off"] + rows * cols] = True
            if it["dstT_off"] < 0:
                continue
            blkT = gotT[it["dstT_off"]:it["dstT_off"] + cols * ldt].view(cols, ldt)
            ok = _matches_torch_rounding(blkT[:, :rows], x.T.contiguous())
            assert bool(ok.all()), (j, "transposed", ok.logical_not().nonzero()[:8].tolist())
            padc = blkT[:, rows:]
            assert bool(((padc == fill) | (padc == 0)).all()), (j, "pad columns hold something other than zeros")
            if zeroed:                                             # the documented usage: the block IS the zero-padded transpose
                assert int((padc != 0).sum()) == 0
            seenT[it["dstT_off"]:it["dstT_off"] + cols * ldt] = True
        assert bool((got[~seen] == SENTINEL).all()) and bool((gotT[~seenT] == fill).all())       # nothing outside the items,
        assert int((~seenT).sum()) == 2 + 2 * (1 + 2 + 3 + 5 + 6)                                # and the skipped item nowhere


# ------------------------------------------------------------------------------------------- 5. sums of squares, mse backward
N_BIG = 16_777_216 + 5          # past the 1024-workgroup cap of the 16-byte form: 17 units for lane 0, the four-deep loop runs four times


@pytest.fixture(scope="module")
def big_gradient():
    """64 MB of gradients and the fp64 sum of their squares, made once"""
    x = torch.randn(N_BIG, generator=torch.Generator().manual_seed(71))
    return x, float((x.double() ** 2).sum())


def _sumsq_case(x, want, off=0):
    """m324_grad_sumsq on x (at `off` elements past a 16-byte boundary): plain, accumulated, and with non-finite values at the
    first element, the last, the n % 4 tail and the last 16-byte unit: left bit-identical by sanitize=False, replaced by sanitize=True"""
    from motion324_amd import ops
    n = x.numel()
    # the elements at the edges of the access pattern weigh 900 each, far more than the bound even at 16 M elements of variance 1:
    # a sum that leaves one of them out cannot pass
    spots = sorted({0, n - 1, (n // 4) * 4 if n % 4 else n - 1, max((n // 4) * 4 - 1, 0)})
    x = x.clone()
    want -= float((x[spots].double() ** 2).sum())
    x[spots] = torch.tensor([30.0, -30.0, 30.0, -30.0])[:len(spots)]
    want += 900.0 * len(spots)
    store = torch.zeros(n + off, device=DEV)
    gd = store[off:]
    gd.copy_(x)
    assert gd.data_ptr() % 16 == 4 * off
    vec, grid, depth = eb.grad_sumsq_plan(n, off == 0)
    out, partial = torch.full((), 123.0, device=DEV), torch.empty(1024, device=DEV)
    bound = eb.sum_of_squares(want, n, depth)
    ratios = {}
    ops.grad_sumsq(gd, out, partial, sanitize=False, accumulate=False)
    ratios["sum"] = eb.assert_within(out, _t(want), _t(bound), f"grad_sumsq n {n}")
    assert torch.equal(_bits(gd), _bits(x))
    first = float(out)
    ops.grad_sumsq(gd, out, partial, sanitize=True, accumulate=True)
    ratios["accumulated"] = eb.assert_within(out, _t(first + want), _t(bound + U * (first + want + bound)), f"grad_sumsq n {n} accumulate")
    assert torch.equal(_bits(gd), _bits(x))                       # nothing to sanitise: nothing written
    bad = x.clone()
    for k, i in enumerate(spots):
        bad[i] = (float("nan"), float("inf"), float("-inf"))[k % 3]
    clean = torch.nan_to_num(bad, nan=0.0, posinf=1e-6, neginf=-1e-6)
    want2 = want - float((x[spots].double() ** 2).sum()) + float((clean[spots].double() ** 2).sum())
    gd.copy_(bad)
    ops.grad_sumsq(gd, out, partial, sanitize=False, accumulate=False)      # the flag is obeyed: the non-finite values stay (the sum is NaN)
    assert torch.equal(_bits(gd), _bits(bad))
    ops.grad_sumsq(gd, out, partial, sanitize=True, accumulate=False)
    assert torch.equal(_bits(gd), _bits(clean))
    ratios["sanitised"] = eb.assert_within(out, _t(want2), _t(eb.sum_of_squares(want2, n, depth)), f"grad_sumsq n {n} sanitised")
    _record(f"grad_sumsq n {n} offset {off} ({'16-byte' if vec else 'scalar'} form, {grid} workgroups, depth {depth})", ratios)


@pytest.mark.parametrize("n,off", [(1, 0), (4095, 0), (4096, 0), (4096, 1), (4096 + 3, 0)])
def test_grad_sumsq_at_the_switch_to_the_16_byte_form(n, off):
    x = torch.randn(n, generator=torch.Generator().manual_seed(72 + n))
    _sumsq_case(x, float((x.double() ** 2).sum()), off)


def test_grad_sumsq_past_the_workgroup_cap(big_gradient):
    _sumsq_case(*big_gradient)


@pytest.mark.parametrize("n", [1, 255, 262_144 + 1, 3_000_017])
def test_mse_against_fp64(n):
    """one element, one workgroup, the first size past the 1024-workgroup cap (one lane takes a second element), a few million"""
    from motion324_amd import ops
    a = torch.randn(n, generator=torch.Generator().manual_seed(81))
    b = a + 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(82))
    total = float(((a.double() - b.double()) ** 2).sum())
    grid, depth = eb.mse_plan(n)
    ratios = {}
    for w in (1.0, 0.5):
        # (a - b)^2: the difference twice and the product; behind the sum (float)n, the quotient and the product with the weight
        bound = w / n * eb.sum_of_squares(total, n, depth, term_roundings=3, post_roundings=3) + eb.TINY32
        out = ops.mse(a.to(DEV), b.to(DEV), w)
        ratios[f"weight {w}"] = eb.assert_within(out, _t(w * total / n), _t(bound), f"mse n {n} weight {w}")
    _record(f"mse n {n} ({grid} workgroups, depth {depth})", ratios)


@pytest.mark.parametrize("gs", [None, 0.37])
def test_mse_bwd_against_fp64(gs):
    """n past 4096 * 256 (the grid-stride loop), element by element: d = (coef gs) (pred - target) is three roundings; exactly 0
    where pred == target"""
    from motion324_amd import ops
    n, w = 4096 * 256 + 256 + 7, 0.5
    a = torch.randn(n, generator=torch.Generator().manual_seed(91))
    e = torch.randn(n, generator=torch.Generator().manual_seed(92))
    b = a + torch.sign(e) * (0.05 + 0.1 * e.abs())              # never so close that the fp32 sum rounds back to a
    same = torch.arange(0, n, 1001).tolist() + [n - 1, 4096 * 256, 4096 * 256 - 1]
    b[same] = a[same]
    d = ops.mse_bwd(a.to(DEV), b.to(DEV), w, _scalar(gs)).cpu()
    coef = eb.f32(2.0 * w / n) * (1.0 if gs is None else eb.f32(gs))
    ref = coef * (a.double() - b.double())
    bound = eb._gamma(3) * ref.abs() + 2 * eb.TINY32
    _record(f"mse_bwd n {n} gs {gs}", {"d": eb.assert_within(d, ref, bound, f"mse_bwd gs {gs}")})
    assert bool((d[same] == 0).all()) and int((d == 0).sum()) == len(set(same))
