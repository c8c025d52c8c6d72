"""Every bf16 GEMM call of tests/golden/gemm_dispatch_table.json goes to the tile kernel the table records for it."""
import json
import os

import pytest

import gemm_dispatch_cases as cases

ENTRIES = {"mp_gemm_bf16_nt", "mp_gemm_qkv_rope_bf16", "mp_gemm_qkv_rope_scaled_bf16", "mp_gemm_qkv_rope_bounded_bf16",
           "mp_gemm_qkv_rope_scaled_bounded_bf16", "mp_gemm_swiglu_keep_bf16", "mp_gemm_bf16_nt_batched", "mp_gemm_bf16_nt_batched_res",
           "mp_gemm_bf16_nt_batched_rows", "mp_gemm_bf16_nt_batched_rows_scaled"}


@pytest.mark.gpu
def test_gemm_dispatch_matches_recorded_table(dev, golden_dir):
    """The table was written by scripts/make_gemm_dispatch_table.py on an MI355X at the commit before the host dispatch moved into
    gemm_dispatch.cpp: the calls one MoE training step, one LoRA step, the CLIP and SAM towers and evaluate() issue (7B dimensions, 2 layers,
    B = 8), the shapes of the selection tests in test_gpu_trunk_kernels.py, and every entry point under tile policies -1, 0 and 2.  Each row is
    issued again (tests/gemm_dispatch_cases.py: zero operands, the row's sizes, epilogue, policy and stream) and ops.gemm_last_kernel() must
    report the recorded tile.  The table itself must hold every entry point and all three tiles, or the replay proves nothing."""
    with open(os.path.join(golden_dir, "gemm_dispatch_table.json")) as f:
        table = json.load(f)
    assert {r["entry"] for r in table} == ENTRIES
    assert {r["tile"] for r in table} == {128, 256, 320}
    assert any(r["source"] == "product" for r in table) and any(r["stream"] == "side" for r in table)
    wrong = []
    for r in table:
        got = cases.replay(r, dev)
        if got != r["tile"]:
            wrong.append((got, r))
    assert not wrong, f"{len(wrong)} of {len(table)} calls changed kernel: {wrong[:5]}"


@pytest.mark.gpu
def test_kept_gate_up_on_a_registered_stream_does_not_count_on_the_subwave_split(dev):
    """The one call whose kernel depends on dispatch_gemm() handing the stream to the selection model for every dense entry: a kept-gate|up
    GEMM of half a wave of 320-row tiles with a long K (2556 x 4096 x 11008: 8 x 16 = 128 tiles).  On the primary stream the model counts on
    the two-way K split and takes the 320-row kernel; a stream with its own registered workspace never splits (mp_launch_gemm320), so there
    the model must not assume the split either and the call stays on 256-row tiles -- what mp_gemm_bf16_nt gets for the same sizes (the
    2556 x 4096 x 11008 side-stream row of the table)."""
    keep = cases.row("mp_gemm_swiglu_keep_bf16", 2556, 4096, 11008, act=5)
    assert cases.replay(keep, dev) == 320
    assert cases.replay(dict(keep, stream="side"), dev) == 256
    assert cases.replay(cases.row("mp_gemm_bf16_nt", 2556, 4096, 11008, stream="side"), dev) == 256
