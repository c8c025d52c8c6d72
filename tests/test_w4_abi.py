"""CPU: the NF4 decode-weight entry points (block-wise quantiser, 4-bit-weight GEMV) are declared in include/medplib_hip.h, exported by the
library and refuse bad arguments before any launch; ops.*w4 refuse CPU tensors; and the torch restatement of the format the GPU tests
compare against (tests/nf4_ref.py) checks itself."""
import ctypes
import os

import pytest
import torch

import nf4_ref as R
from medplib_amd import _lib

NEW = ("mp_quantize_blocks_nf4_bf16", "mp_gemv_w4_bf16")
P = 4096                      # any non-null address: every refusal below comes before a launch


def test_header_declares_and_library_exports_the_w4_entry_points():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def _gemv(L, M=1, N=256, K=512, act=0, bias=None, residual=None, x=P, codes=P, absmax=P, y=P, out_dtype=0, ldw=None, lda=None, w_index=None):
    return L.raw("mp_gemv_w4_bf16")(x, K, codes, K // 2 if ldw is None else ldw, 0, absmax, K // 64 if lda is None else lda, 0, y, N, bias, residual,
                                    N, w_index, None, None, M, N, K, act, out_dtype, 1.0, None)


def test_gemv_w4_refuses_before_any_launch():
    L = _lib.lib()
    for M in (0, 9):
        assert _gemv(L, M=M) == -1 and "mp_gemv_w4_bf16" in L.last_error() and "M <= 8" in L.last_error()
    for K in (32, 96, 16 * 33):
        assert _gemv(L, K=K, ldw=512, lda=64) == -1 and "K % 64" in L.last_error()
    assert _gemv(L, ldw=264) == -1 and "ldw_bytes % 16" in L.last_error()           # a row stride the 16-byte loads cannot take
    assert _gemv(L, ldw=240) == -1 and "ldw_bytes" in L.last_error()                # rows that overlap
    assert _gemv(L, lda=7) == -1 and "lda >= K / 64" in L.last_error()
    assert _gemv(L, bias=P) == -5 and "bias" in L.last_error()
    for act in (1, 2, 3, 4, 6, -1):                            # RELU, GELU, QUICK_GELU, SILU, ROPE_QK, nonsense
        assert _gemv(L, act=act) == -5 and "NONE or SWIGLU_PAIR" in L.last_error()
    assert _gemv(L, act=5, N=1000) == -5 and "N % 64" in L.last_error()
    assert _gemv(L, act=5, N=256, residual=P) == -5 and "no residual" in L.last_error()
    assert _gemv(L, act=5, N=256, out_dtype=1) == -5 and "bf16 output" in L.last_error()
    assert _gemv(L, w_index=P, out_dtype=1) == -5 and "indexed" in L.last_error()
    assert _gemv(L, out_dtype=7) == -2
    for null in ("x", "codes", "absmax", "y"):
        assert _gemv(L, **{null: None}) == -5 and "null operand" in L.last_error()


def test_quantizer_refuses_before_any_launch():
    L = _lib.lib()
    q = L.raw("mp_quantize_blocks_nf4_bf16")            # (W, ldw, rows, K, codes, ldc_bytes, absmax, lda, stream)
    assert q(P, 512, 0, 512, P, 256, P, 8, None) == -1 and "mp_quantize_blocks_nf4_bf16" in L.last_error()      # no rows
    assert q(P, 96, 4, 96, P, 48, P, 2, None) == -1 and "K % 64" in L.last_error()
    assert q(P, 256, 4, 512, P, 256, P, 8, None) == -1           # ldw < K
    assert q(P, 512, 4, 512, P, 255, P, 8, None) == -1           # ldc_bytes < K / 2
    assert q(P, 512, 4, 512, P, 256, P, 7, None) == -1           # lda < K / 64
    for args in ((None, 512, 4, 512, P, 256, P, 8, None), (P, 512, 4, 512, None, 256, P, 8, None), (P, 512, 4, 512, P, 256, None, 8, None)):
        assert q(*args) == -5 and "null operand" in L.last_error()


def test_ops_w4_refuse_cpu_tensors():
    from medplib_amd import ops
    x = torch.zeros(1, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.gemv_w4(x, torch.zeros(16, 32, dtype=torch.uint8), torch.zeros(16, 1))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.quantize_blocks_nf4(torch.zeros(16, 64, dtype=torch.bfloat16))


def test_model_api_has_the_4bit_pair_and_the_worker_points_to_it():
    from medplib_amd.model.generation import GenerationMixin
    from medplib_amd.model.llama import LlamaStack
    from model.serve import model_worker as MW
    assert isinstance(GenerationMixin.decode_4bit, property) and callable(GenerationMixin.enable_decode_4bit)
    for name in ("quantize_decode_weights", "drop_decode_weights", "decode_weights_unsupported"):
        assert callable(getattr(LlamaStack, name))
    with pytest.raises(ValueError, match="enable_decode_4bit") as e:
        MW.check_placement(MW.parse_args(["--model-path", "checkpoints/tiny", "--device_map", "cuda", "--load-4bit"]))
    assert "bf16" in str(e.value)


# ---------------------------------------------------------------- the reference restatement checks itself
def test_reference_table_and_thresholds():
    assert R.NF4.dtype == torch.float32 and R.NF4.numel() == 16 and (R.NF4[1:] > R.NF4[:-1]).all()
    assert float(R.NF4[0]) == -1.0 and float(R.NF4[7]) == 0.0 and float(R.NF4[15]) == 1.0
    assert R.THRESHOLDS.dtype == torch.float32 and R.THRESHOLDS.numel() == 15
    assert (R.THRESHOLDS[1:] > R.THRESHOLDS[:-1]).all(), "strictly increasing"
    assert (R.THRESHOLDS > R.NF4[:-1]).all() and (R.THRESHOLDS < R.NF4[1:]).all()
    assert R.NF4_BF16.unique().numel() == 16, "the bf16 rounding keeps the sixteen values distinct"
    assert torch.equal(R.NF4_BF16.to(torch.bfloat16).float(), R.NF4_BF16)


def test_reference_quantiser_returns_every_code_on_the_grid():
    """quant_ref(bf16(NF4[c]) * 2^e) returns c: a block that holds all sixteen table values (so its absmax is 2^e exactly)."""
    for e in (-7, -6, 0, 3):
        code = torch.arange(64) % 16
        w = (R.NF4_BF16[code] * 2.0 ** e).to(torch.bfloat16).unsqueeze(0)
        assert torch.equal(w.float(), (R.NF4_BF16[code] * 2.0 ** e).unsqueeze(0))
        got, absmax = R.quant_codes(w)
        assert torch.equal(got[0].long(), code) and float(absmax[0, 0]) == 2.0 ** e
        packed, _ = R.quant_ref(w)
        assert torch.equal(R.dequant_ref(packed, absmax), w.float())


def test_reference_pack_order_ties_and_zero_block():
    code = torch.tensor([[3, 12] + [7] * 62], dtype=torch.uint8)
    packed = R.pack(code)
    assert packed.shape == (1, 32) and int(packed[0, 0]) == (3 << 4 | 12), "the high nibble is the even k"
    assert torch.equal(R.unpack(packed), code)
    z = torch.zeros(2, 128, dtype=torch.bfloat16)
    c, a = R.quant_ref(z)
    assert (c == 0x77).all() and (a == 0).all()
    # a value exactly on a threshold goes to the lower code (fp32 weights, block absmax 1: v = w), the next fp32 above it to the upper one
    w = torch.zeros(1, 64)
    w[0, 0] = 1.0
    w[0, 1:16] = R.THRESHOLDS
    got, _ = R.quant_codes(w)
    assert torch.equal(got[0, 1:16].long(), torch.arange(15)), "strict comparison: a tie takes the lower code"
    w[0, 1:16] = torch.nextafter(R.THRESHOLDS, torch.tensor(2.0))
    got, _ = R.quant_codes(w)
    assert torch.equal(got[0, 1:16].long(), torch.arange(1, 16))


def test_no_bf16_weight_lands_exactly_on_a_threshold():
    """Why the GPU quantiser tests bracket the thresholds instead of hitting them: the quantiser takes bf16 weights, and for no bf16 pair
    (w, absmax) is fp32(w * fp32(1 / absmax)) one of the fifteen thresholds.  Exhaustive: every absmax mantissa (the exponent only scales
    w) against every finite bf16 w with |w| <= absmax.  The tie rule is therefore checked on the fp32 restatement above, and on the GPU by
    the nearest bf16 weights on either side of every threshold (tests/test_gpu_w4_gemv.py)."""
    allbf = (torch.arange(0, 65536, dtype=torch.int32) << 16).view(torch.float32)
    allbf = allbf[torch.isfinite(allbf)]
    for a in allbf[(allbf >= 1) & (allbf < 2)]:
        v = allbf[allbf.abs() <= a] * (torch.tensor(1.0) / a)
        assert not torch.isin(v, R.THRESHOLDS).any(), float(a)
