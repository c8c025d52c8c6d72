"""CPU: the grouped top-2 expert GEMVs (mp_gemv_grouped_top2_gate_up_bf16, mp_gemv_grouped_top2_down_bf16) are declared in
include/medplib_hip.h, exported by the library and refuse bad arguments before any launch, each with its own name in the message; the two ops
wrappers refuse CPU tensors."""
import ctypes
import os

import pytest
import torch

from medplib_amd import _lib

GATE_UP, DOWN = "mp_gemv_grouped_top2_gate_up_bf16", "mp_gemv_grouped_top2_down_bf16"
NEW = (GATE_UP, DOWN)
P = 4096                      # any non-null address: every refusal below comes before a launch
SHAPE, ARG = -1, -5           # MP_ERR_SHAPE, MP_ERR_ARG


def test_header_declares_and_library_exports_the_grouped_top2_entry_points():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def _gate_up(L, tokens=2, N=256, K=512, E=3, x=P, W=P, act=P, expert=P, slot=P, ldx=None, ldw=None, stride_w=None, ldact=None):
    ldw = K if ldw is None else ldw
    return L.raw(GATE_UP)(x, K if ldx is None else ldx, W, ldw, N * ldw if stride_w is None else stride_w, act, N // 2 if ldact is None else ldact,
                          expert, slot, tokens, N, K, E, None)


def _down(L, tokens=2, N=256, K=512, E=3, act=P, W=P, y=P, residual=P, expert=P, slot=P, weight=P, ldact=None, ldw=None, stride_w=None, ldy=None,
          ldr=None):
    ldw = K if ldw is None else ldw
    return L.raw(DOWN)(act, K if ldact is None else ldact, W, ldw, N * ldw if stride_w is None else stride_w, y, N if ldy is None else ldy, residual,
                       N if ldr is None else ldr, expert, slot, weight, tokens, N, K, E, None)


@pytest.mark.parametrize("name,call,operands", [(GATE_UP, _gate_up, ("x", "W", "act", "expert", "slot")),
                                                (DOWN, _down, ("act", "W", "y", "expert", "slot", "weight"))])
def test_grouped_top2_gemvs_refuse_before_any_launch(name, call, operands):
    L = _lib.lib()

    def refused(code, words, **kw):
        assert call(L, **kw) == code, (kw, L.last_error())
        assert L.last_error().startswith(name + ":") and words in L.last_error(), (kw, L.last_error())

    for tokens in (0, 9):
        refused(SHAPE, "tokens <= 8", tokens=tokens)
    for E in (0, -1):
        refused(SHAPE, "E >= 1", E=E)
    for K in (4, 516):
        refused(SHAPE, "K % 8", K=K, ldw=520, **({"ldx": 520} if name == GATE_UP else {"ldact": 520}))
    refused(SHAPE, "ld* % 8", ldw=516)
    refused(SHAPE, "ld* % 8", stride_w=256 * 512 + 4)
    refused(SHAPE, "ld* % 8", **({"ldx": 516} if name == GATE_UP else {"ldact": 516}))
    if name == GATE_UP:
        for N in (1000, 32):
            refused(SHAPE, "N % 64", N=N, ldact=512)
        refused(SHAPE, "ldact >= N / 2", ldact=127)
    else:
        refused(SHAPE, "ldy >= N", ldy=255)
        refused(SHAPE, "ldr >= N", ldr=255)
    for null in operands:
        refused(ARG, "null operand", **{null: None})


def test_grouped_top2_ops_refuse_cpu_tensors():
    from medplib_amd import ops
    T, d, ff, E = 2, 64, 64, 3
    h, act, res = torch.zeros(T, d, dtype=torch.bfloat16), torch.zeros(2 * T, ff, dtype=torch.bfloat16), torch.zeros(T, d, dtype=torch.bfloat16)
    expert, slot, weight = torch.zeros(2 * T, dtype=torch.int32), torch.zeros(2 * T, dtype=torch.int32), torch.zeros(2 * T)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.gemv_grouped_top2_gate_up(h, torch.zeros(E, 2 * ff, d, dtype=torch.bfloat16), expert, slot)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.gemv_grouped_top2_down(act, torch.zeros(E, d, ff, dtype=torch.bfloat16), expert, slot, weight, res)
