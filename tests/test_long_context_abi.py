"""CPU: the bounded RoPE / KV-append entry points of long sequences are declared in include/medplib_hip.h, exported by the library and refuse
out-of-table positions and null operands before any launch; LlamaStack.ensure_positions grows the RoPE tables past max_position_embeddings
with the rows already in use unchanged (no GPU needed)."""
import ctypes
import os
import types

import torch

from medplib_amd import _lib
from medplib_amd.model.llama import LlamaStack, ROPE_GROW_ROWS, _rope_tables, rope_rows_for
from oracle import ops as O

NEW = ("mp_rope_qk_bounded_bf16", "mp_gemm_qkv_rope_bounded_bf16", "mp_gemm_qkv_rope_scaled_bounded_bf16",
       "mp_decode_rope_append_bounded_bf16", "mp_gemv_rmsnorm_rope_append_bounded_bf16")
FAKE = 64            # a non-null address: every call below is refused before it would be dereferenced or launched


def test_header_declares_and_library_exports_the_bounded_entry_points():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    assert [a for _, a in protos["mp_decode_rope_append_bounded_bf16"][1][-4:]] == ["table_rows", "cache_rows", "err", "stream"]
    assert [a for _, a in protos["mp_rope_qk_bounded_bf16"][1][-2:]] == ["table_rows", "stream"]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def test_prefill_rope_refuses_positions_past_the_table():
    L = _lib.lib()
    rope = L.raw("mp_rope_qk_bounded_bf16")
    #          qkv   ld     cos   sin   tokens seq   H   D    pos0 rows
    assert rope(FAKE, 12288, FAKE, FAKE, 4700, 4700, 32, 128, 0, 4096, None) == -1
    assert "table_rows = 4096" in L.last_error() and "4700" in L.last_error()
    assert rope(FAKE, 12288, FAKE, FAKE, 1, 1, 32, 128, 4096, 4096, None) == -1          # one decode row at position 4096
    assert rope(FAKE, 12288, FAKE, FAKE, 1, 1, 32, 128, -1, 4096, None) == -1           # negative offset
    assert rope(None, 12288, FAKE, FAKE, 1, 1, 32, 128, 0, 4096, None) == -5 and "null operand" in L.last_error()
    assert rope(FAKE, 12288, FAKE, None, 1, 1, 32, 128, 0, 4096, None) == -5
    for name in ("mp_gemm_qkv_rope_bounded_bf16", "mp_gemm_qkv_rope_scaled_bounded_bf16"):
        fn = L.raw(name)
        scaled = "scaled" in name
        args = lambda cos, seq, pos0, rows: ((FAKE, 4096, FAKE, 4096, FAKE, 12288, cos, FAKE) + ((FAKE,) if scaled else ())
                                             + (seq, 12288, 4096, seq, pos0, 128, rows, None))
        assert fn(*args(FAKE, 4700, 0, 4096)) == -1 and name in L.last_error() and "table_rows = 4096" in L.last_error()
        assert fn(*args(FAKE, 2048, 2049, 4096)) == -1                                    # seq + pos_offset = 4097
        assert fn(*args(None, 16, 0, 4096)) == -5 and "null" in L.last_error()


def test_decode_entry_points_refuse_missing_bounds_and_error_word():
    L = _lib.lib()
    dec = L.raw("mp_decode_rope_append_bounded_bf16")
    #                 qkv   ld     cos   sin   ck    cv    pos   B  H   D    c_sb          c_ss  rows  cache err
    assert dec(FAKE, 12288, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 32, 128, 9216 * 4096, 4096, 0, 9216, FAKE, None) == -1
    assert "table_rows" in L.last_error()
    assert dec(FAKE, 12288, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 32, 128, 9216 * 4096, 4096, 9216, 0, FAKE, None) == -1
    assert dec(FAKE, 12288, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 32, 128, 9216 * 4096, 4096, 9216, 9216, None, None) == -5
    assert "null operand" in L.last_error()
    assert dec(FAKE, 12288, None, FAKE, FAKE, FAKE, FAKE, 1, 32, 128, 9216 * 4096, 4096, 9216, 9216, FAKE, None) == -5
    gv = L.raw("mp_gemv_rmsnorm_rope_append_bounded_bf16")

    def gcall(rows, cache_rows, err, cos=FAKE):
        return gv(FAKE, 4096, FAKE, 1e-5, FAKE, 4096, FAKE, 12288, cos, FAKE, FAKE, FAKE, FAKE, 1, 32, 128, 4096, 9216 * 4096, 4096,
                  rows, cache_rows, err, None)
    assert gcall(0, 9216, FAKE) == -1 and "table_rows" in L.last_error()
    assert gcall(9216, 9216, None) == -5 and "null operand" in L.last_error()
    assert gcall(9216, 9216, FAKE, cos=None) == -5 and "null operand" in L.last_error()


def _stack(rows, lora=False):
    cfg = types.SimpleNamespace(head_dim=128, rope_theta=10000.0, max_position_embeddings=rows)
    cos, sin = _rope_tables(rows, 128, 10000.0, "cpu")
    return types.SimpleNamespace(cfg=cfg, device="cpu", cos=cos, sin=sin, sin_neg=(-sin).contiguous() if lora else None)


def test_grown_tables_keep_their_rows_and_follow_the_reference_formula():
    st = _stack(4096, lora=True)
    cos0, sin0 = st.cos, st.sin
    LlamaStack.ensure_positions(st, 4096)                                     # covered: nothing happens
    assert st.cos is cos0 and st.sin is sin0
    LlamaStack.ensure_positions(st, 4700)
    assert st.cos.shape == (5120, 64) and st.sin.shape == (5120, 64) and st.cos.is_contiguous()
    assert torch.equal(st.cos[:4096], cos0) and torch.equal(st.sin[:4096], sin0)
    assert torch.equal(st.sin_neg, -st.sin)                                   # the LoRA backward's table follows
    ref_cos, ref_sin = O.rope_tables(5120, 128)                               # the oracle (HF 4.31's fp32 formula) at the grown length
    assert torch.allclose(st.cos, ref_cos, rtol=0, atol=1e-6) and torch.allclose(st.sin, ref_sin, rtol=0, atol=1e-6)
    fresh_cos, _ = _rope_tables(4096, 128, 10000.0, "cpu")
    assert torch.equal(st.cos[:4096], fresh_cos)
    LlamaStack.ensure_positions(st, 8193)
    assert st.cos.shape[0] == 9216 and torch.equal(st.cos[:5120], torch.cat([cos0, st.cos[4096:5120]]))


def test_growth_rounds_up_to_whole_blocks():
    assert ROPE_GROW_ROWS == 1024
    assert rope_rows_for(4096, 4096) == 4096 and rope_rows_for(10, 4096) == 4096            # never shrinks
    assert rope_rows_for(4097, 4096) == 5120 and rope_rows_for(5120, 4096) == 5120
    assert rope_rows_for(8192 + 24, 4096) == 9216
    assert rope_rows_for(8180 + 24, 8192) == 9216                                        # the decode test's second prompt
    assert rope_rows_for(70, 64) == 1024                                                 # tiny configs grow to one block
