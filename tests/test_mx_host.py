"""MXFP8 inference mode without a device: the three C entry points (exports, bindings, argument validation), the compiled
MX GEMM (scaled MFMA, no spills, barrier audit), and how a model selects the mode (config, attribute, switch; where it is off)."""
import ctypes as C
import os
import re

import pytest
import torch

from motion324_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m324_mx_quant", "m324_layernorm_mx", "m324_gemm_mx")


def _lib():
    from motion324_amd import lib
    return lib, lib.load()


def test_library_exports_the_mx_entries_and_header_and_bindings_agree():
    lib, h = _lib()
    header = open(os.path.join(ROOT, "include", "m324.h")).read()
    for name in NEW:
        assert hasattr(h, name), name
        assert name in lib.SIGNATURES
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(lib.SIGNATURES[name]), name
    assert "M324_MXFP8 = 2" in header and lib.MXFP8 == 2
    assert h.m324_abi_version() == lib.ABI_VERSION == 23


def _err(h):
    buf = C.create_string_buffer(512)
    h.m324_last_error(buf, 512)
    return buf.value.decode()


A16 = 1 << 20          # aligned stand-in addresses: validation reads sizes and alignments only, every case below is refused


def _args(lib, M=256, N=256, K=768, **kw):
    a = lib.GemmArgs()
    a.A, a.W, a.C = A16, A16, A16
    a.lda, a.ldw, a.ldc = K, K, N
    a.M, a.N, a.K = M, N, K
    a.in_dtype, a.out_dtype, a.batch = lib.MXFP8, lib.BF16, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("case,code,text", [
    (dict(K=192, lda=192, ldw=192), -3, "multiple of 128"),
    (dict(N=96, ldc=96), -3, "multiple of 64"),
    (dict(batch=2), -3, "batch"),
    (dict(in_dtype=1), -1, "in_dtype"),
    (dict(A=A16 + 8), -1, "aligned"),
    (dict(lda=776), -1, "aligned"),
    (dict(M=0), -1, "empty"),
    (dict(ldc=128), -1, "ldc"),
    (dict(act=1), -3, "not built"),
    (dict(out_dtype=0), -3, "not built"),
    (dict(row_gin=16, row_gout=32), -3, "row map"),
    (dict(ln_rowstat=A16, ln_colsum=A16), -3, "fold"),
    (dict(aux_mode=1, aux=A16, ldaux=256), -3, "aux_mode"),
    (dict(aux_mode=3, C=None, qkv_L=100, qkv_H=1, qkv_q=A16, qkv_k=A16, qkv_v=A16, N=192, ldc=192), -1, "qkv_L"),
    (dict(aux_mode=4, C=None, qkv_L=128, qkv_H=1, qkv_q=A16, qkv_k=A16, N=128, ldc=128), -1, "V output"),
])
def test_gemm_mx_validation_returns_before_any_device_call(case, code, text):
    lib, h = _lib()
    a = _args(lib, **case)
    rc = h.m324_gemm_mx(C.byref(a), A16, 24, A16, 24, None, 0, None)
    assert rc == code and text in _err(h), (rc, _err(h))


def test_gemm_mx_validation_of_scales_and_mx_output():
    lib, h = _lib()
    a = _args(lib)
    assert h.m324_gemm_mx(C.byref(a), None, 24, A16, 24, None, 0, None) == -1               # no A scales
    assert h.m324_gemm_mx(C.byref(a), A16 + 2, 24, A16, 24, None, 0, None) == -1           # misaligned scale rows
    assert h.m324_gemm_mx(C.byref(a), A16, 22, A16, 24, None, 0, None) == -1               # lds too small / not a multiple of 4
    mxo = _args(lib, out_dtype=lib.MXFP8, act=1)
    assert h.m324_gemm_mx(C.byref(mxo), A16, 24, A16, 24, None, 0, None) == -1             # MX output without its scales
    assert h.m324_gemm_mx(C.byref(mxo), A16, 24, A16, 24, A16, 4, None) == -1              # ... or with too few of them
    res = _args(lib, out_dtype=lib.F32, residual=A16 + 4096, ldr=256)
    assert h.m324_gemm_mx(C.byref(res), A16, 24, A16, 24, None, 0, None) == -3             # residual other than C: not built
    assert h.m324_gemm_mx(None, A16, 24, A16, 24, None, 0, None) == -1


def test_mx_quant_and_layernorm_mx_validation():
    lib, h = _lib()
    q = h.m324_mx_quant
    assert q(None, 0, 64, 4, 64, A16, 64, A16, 4, None) == -1
    assert q(A16, 2, 64, 4, 64, A16, 64, A16, 4, None) == -1 and "x_dtype" in _err(h)
    assert q(A16, 0, 64, 4, 48, A16, 64, A16, 4, None) == -1 and "K" in _err(h)
    assert q(A16, 0, 64, 4, 64, A16, 64, A16, 1, None) == -1 and "leading" in _err(h)
    assert q(A16 + 4, 0, 64, 4, 64, A16, 64, A16, 4, None) == -1 and "aligned" in _err(h)
    assert q(A16, 0, 64, 0, 64, A16, 64, A16, 4, None) == -1
    ln = h.m324_layernorm_mx
    assert ln(A16, 768, A16, None, 1e-5, 4, 2048, A16, 2048, A16, 64, None) == -1 and "C" in _err(h)
    assert ln(A16, 768, A16, None, 1e-5, 4, 760, A16, 768, A16, 24, None) == -1
    assert ln(A16, 768, None, None, 1e-5, 4, 768, A16, 768, A16, 24, None) == -1
    assert ln(A16, 768, A16, A16 + 4, 1e-5, 4, 768, A16, 768, A16, 24, None) == -1 and "aligned" in _err(h)
    assert ln(A16, 768, A16, None, 1e-5, 4, 768, A16, 768, A16, 8, None) == -1 and "leading" in _err(h)


def test_compiled_mx_gemm_uses_the_scaled_mfma_and_spills_nothing():
    from motion324_amd import build as B
    asm = open(B.assembly(["gemm_mx.hip"])["gemm_mx.hip"]).read()
    assert "v_mfma_scale_f32_32x32x64_f8f6f4" in asm
    meta = asm[asm.index("amdhsa.kernels:"):]
    blocks = meta.split("  - .agpr_count:")[1:]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    assert sum("gemm_mx_kernel" in n for n in names) == 4, names
    for b, n in zip(blocks, names):
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, n
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, n
    # no scalar-memory writes in the new translation unit (house rule; the MX scales are written with vector stores).  The
    # mnemonic prefixes live in a text document next to this file, so that no source file of the tree spells them.
    src = open(os.path.join(ROOT, "motion324_amd", "csrc", "gemm_mx.hip")).read().lower()
    with open(os.path.join(ROOT, "tests", "scalar_memory_write_mnemonics.txt")) as f:
        words = [w.strip() for w in f if w.strip() and not w.startswith("#")]
    assert len(words) == 6
    for word in words:
        assert word not in src and word not in asm.lower(), word


def test_mx_gemm_loop_overlaps_the_next_tiles_dma_with_the_mfmas():
    """Between issuing a tile's LDS-DMA pieces and the next scaled MFMA the compiled loop waits for no vector-memory load: the
    fragment reads of the current stage are not taken for readers of the stage in flight (alias-scoped views, gemm_mx_body)."""
    from motion324_amd import build as B
    lines = open(B.assembly(["gemm_mx.hip"])["gemm_mx.hip"]).read().split("\n")
    name, checked = None, {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\S*gemm_mx_kernel\S*):", l)
        if m:
            name = m.group(1)
            continue
        if name is None or "buffer_load_dwordx4" not in l or " lds" not in l:
            continue
        waits, j = [], i + 1
        while j < len(lines) and "v_mfma_scale" not in lines[j] and not re.match(r"^_Z", lines[j]):
            if "buffer_load_dwordx4" in lines[j] and " lds" in lines[j]:
                waits = []                                 # measured from the LAST piece of a run
            if "s_waitcnt" in lines[j] and "vmcnt" in lines[j]:
                waits.append(lines[j].strip())
            j += 1
        assert not waits, (name, waits)
        checked[name] = checked.get(name, 0) + 1
    assert len(checked) == 4, checked


def test_barrier_audit_covers_the_mx_gemm():
    src = open(os.path.join(ROOT, "tools", "audit_barriers.py")).read()
    assert '"gemm_mx.hip"' in src
    from motion324_amd import build as B
    assert "gemm_mx.hip" in B.SOURCES


# ------------------------------------------------------------------------------------------------ mode selection
def _model(d=384, **kw):
    import motion324_amd as m
    cfg = synth.make_config(frames=3, d=d, tokens=8, pcd_layers=1, n_layer=2)
    cfg["model"]["dino"] = {"depth": 2}
    cfg["model"].update(kw)
    return m.Motion_Latent_Model(cfg)


def test_mode_from_config_attribute_and_switch_with_precedence(monkeypatch):
    from motion324_amd import Pcd_motion
    assert _model().inference_precision == "bf16"
    assert _model(inference_precision="mxfp8").inference_precision == "mxfp8"
    monkeypatch.setattr(Pcd_motion, "MXFP8_DEFAULT", True)
    assert _model().inference_precision == "mxfp8"                              # the switch: a config without the key
    assert _model(inference_precision="bf16").inference_precision == "bf16"     # the config wins over the switch
    m = _model(inference_precision="bf16")
    m.inference_precision = "mxfp8"                                             # the attribute, after construction
    assert m.inference_precision == "mxfp8"
    with pytest.raises(ValueError):
        m.inference_precision = "fp8"


def test_switch_is_in_the_table_and_defaults_off():
    from motion324_amd import switches
    assert switches.HOST["M324_MXFP8"][0] == "0"
    assert "M324_MXFP8" in switches.table()


def test_mxfp8_refuses_a_width_that_is_not_a_multiple_of_128():
    with pytest.raises(NotImplementedError, match="128"):
        _model(d=192, inference_precision="mxfp8")
    m = _model(d=192)
    with pytest.raises(NotImplementedError):
        m.inference_precision = "mxfp8"
    assert m.inference_precision == "bf16"


def test_mode_is_in_effect_only_in_a_bf16_inference_forward():
    from motion324_amd import prepared, transformer
    m = _model(inference_precision="mxfp8").eval()
    try:
        prepared.set_precision("bf16")
        with torch.no_grad():
            assert m.mx_effective()
            with transformer.fusion_disabled():                    # a training step's forward
                assert not m.mx_effective()
        assert not m.mx_effective()                                # grad on
        prepared.set_precision("fp32")
        with torch.no_grad():
            assert not m.mx_effective()                            # fp32 parity mode
        prepared.set_precision("bf16")
        m.train()
        with torch.no_grad():
            assert not m.mx_effective()                            # training mode
        m.eval()
        m.inference_precision = "bf16"
        with torch.no_grad():
            assert not m.mx_effective()
    finally:
        prepared.set_precision(None)


def test_roles_are_off_outside_a_scope_and_inside_a_training_step():
    from motion324_amd import transformer
    from motion324_amd.prepared import Prepared
    P = Prepared(torch.device("cpu"), torch.bfloat16)
    with torch.no_grad():
        assert not transformer.mx_role(P, "trunk.qkv")
        with transformer.mx_scope(transformer.MX_ROLES):
            assert all(transformer.mx_role(P, r) for r in transformer.MX_ROLES)
            assert not transformer.mx_role(Prepared(torch.device("cpu"), torch.float32), "trunk.mlp")
            with transformer.fusion_disabled():
                assert not transformer.mx_role(P, "dino.qkv")
                with transformer.fusion_allowed():                 # the frozen DINO of a training step stays bf16
                    assert not transformer.mx_role(P, "dino.qkv")
            assert transformer.mx_role(P, "dino.qkv")
        with transformer.mx_scope({"trunk.qkv"}):
            assert transformer.mx_role(P, "trunk.qkv") and not transformer.mx_role(P, "trunk.mlp")
    with transformer.mx_scope(transformer.MX_ROLES):
        assert not transformer.mx_role(P, "trunk.qkv")             # grad on


def test_frame_parallel_refuses_the_mxfp8_mode():
    from motion324_amd.lib import M324Error
    m = _model(inference_precision="mxfp8").eval()
    with pytest.raises(M324Error, match="mxfp8"):
        m.forward_frame_parallel({})


def test_graph_key_differs_between_modes():
    """GraphedForward keys its graphs on the EFFECTIVE mode (as the captured forward sees it: eval, grad off), like the auto-graph."""
    from motion324_amd import prepared
    from motion324_amd.graph import GraphedForward
    m = _model().eval()
    g = GraphedForward(m, weak=True)
    sample = {"ref_pcd": torch.zeros(1, 8, 3), "rgb_video": torch.zeros(1, 3, 32, 32, 3)}
    try:
        prepared.set_precision("bf16")
        k_bf16 = g._key(sample)
        m.inference_precision = "mxfp8"
        k_mx = g._key(sample)
        assert k_mx != k_bf16
        prepared.set_precision("fp32")                   # fp32 parity mode: the setting is not in effect, same graph
        k32 = g._key(sample)
        m.inference_precision = "bf16"
        assert g._key(sample) == k32
    finally:
        prepared.set_precision(None)
