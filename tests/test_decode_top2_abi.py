"""CPU: the top-2 decode entry points (fused norm + gate + top-2 routing, the two-expert GEMVs, the device-keyed gate draws) are declared
in include/medplib_hip.h, exported by the library, and refuse bad shapes before any launch (no GPU needed)."""
import ctypes
import os

from medplib_amd import _lib

NEW = ("mp_decode_norm_gate_route_top2", "mp_gemv_top2_gate_up_bf16", "mp_gemv_top2_down_bf16", "mp_gate_noise_dev_f32")


def test_header_declares_and_library_exports_the_top2_decode_entry_points():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def _route(L, tokens, experts, dim=4096):
    return L.raw("mp_decode_norm_gate_route_top2")(None, dim, None, 1e-5, None, None, dim, None, tokens, dim, experts, 4, None, None, None, None,
                                                   None, None, None)


def test_top2_routing_refuses_bad_shapes():
    L = _lib.lib()
    for tokens, experts in ((9, 3), (0, 3), (4, 9), (4, 0)):
        assert _route(L, tokens, experts) == -1
        assert "mp_decode_norm_gate_route_top2" in L.last_error() and "tokens <= 8" in L.last_error()
    assert _route(L, 4, 3, dim=8200) == -1                    # dim > 8192
    assert _route(L, 4, 3) == -5 and "null operand" in L.last_error()      # shapes pass, the operands are checked next (MP_ERR_ARG)


def test_top2_gemvs_refuse_bad_shapes():
    L = _lib.lib()
    gu = L.raw("mp_gemv_top2_gate_up_bf16")
    assert gu(None, 4096, None, 4096, 4096 * 22016, None, 11008, None, None, 9, 22016, 4096, None) == -1
    assert "tokens <= 8" in L.last_error()
    assert gu(None, 4096, None, 4096, 4096 * 22016, None, 11008, None, None, 2, 22000, 4096, None) == -1       # N % 64 (SwiGLU pairing)
    down = L.raw("mp_gemv_top2_down_bf16")
    assert down(None, 11008, None, 11008, 4096 * 11008, None, 4096, None, 4096, None, None, None, 9, 4096, 11008, None) == -1
    assert "tokens <= 8" in L.last_error()
    assert down(None, 11008, None, 11008, 4096 * 11008, None, 4096, None, 4096, None, None, None, 2, 4096, 11004, None) == -1   # K % 8
    noise = L.raw("mp_gate_noise_dev_f32")
    assert noise(None, 16, 42, None, 16, 1, None) != 0 and "pass_dev" in L.last_error()
