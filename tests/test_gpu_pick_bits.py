"""The three row-pick kernels return the recorded bits: tokens of mp_sample_rows_f32, tokens / kept / cut of mp_sample_filtered_rows_f32 and
every output of mp_beam_topk_f32 on the inputs of tests/pick_bit_cases.py equal tests/golden/pick_bits.npz byte for byte (floats compared
as uint32).  The float64 bands of the other suites would not see a changed rounding order; this does.  The fixture holds results only
(scripts/record_pick_bits.py writes it), and a SHA-256 of every generated input, asserted first: a change of the input generation fails as
itself."""
import os

import numpy as np
import pytest

import pick_bit_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "pick_bits.npz")) as z:
        return {k: z[k] for k in z.files}


def _same_bytes(got, golden, prefix):
    want = {k: v for k, v in golden.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want)
    for k, a in got.items():
        assert a.dtype == want[k].dtype and a.shape == want[k].shape, k
        diff = np.flatnonzero(a.reshape(-1) != want[k].reshape(-1))
        assert a.tobytes() == want[k].tobytes(), (k, len(diff), diff[:8], a.reshape(-1)[diff[:8]], want[k].reshape(-1)[diff[:8]])


def test_generated_inputs_are_the_recorded_ones(golden):
    _same_bytes(cases.input_hashes(), golden, "sha/")


def test_plain_pick_tokens(dev, golden):
    _same_bytes(cases.plain_results(dev), golden, "plain/")


def test_filtered_pick_tokens_kept_and_cut(dev, golden):
    _same_bytes(cases.filtered_results(dev), golden, "filtered/")


def test_beam_candidates_and_selection(dev, golden):
    _same_bytes(cases.beam_results(dev), golden, "beam/")
