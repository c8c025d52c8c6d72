"""What is 8-bit by name among the model tests of the quantised decode modes: the worker's --load-8bit, and the entry-point test of the 8-bit
mode under the name it has always had.  Helpers, the shared body and every other test: tests/test_gpu_quant_decode.py."""
import json

import numpy as np
import pytest
import torch

from test_gpu_quant_decode import KINDS, _tiny, every_decoding_entry_point_runs
from toy_tokenizer import ToyTokenizer  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", KINDS)
def test_every_decoding_entry_point_runs_in_8bit_mode(dev, kind, monkeypatch):
    every_decoding_entry_point_runs(dev, 8, kind, monkeypatch)


class _Tok(ToyTokenizer):
    """The toy tokenizer with a decode: every ordinary id is the piece ' t<id>.', special ids decode to nothing."""

    def decode(self, ids, skip_special_tokens=True):
        special = set(self.special_ids.values()) | {self.bos_token_id, self.eos_token_id, self.pad_token_id}
        return "".join(f" t{i}." for i in ids if not (skip_special_tokens and i in special))


def test_worker_with_load_8bit_streams_the_8bit_answer(dev):
    from model.serve import model_worker as MW
    cfg, m = _tiny(dev, "top1")
    args = MW.parse_args(["--model-path", "checkpoints/tiny", "--device_map", "cuda", "--load-8bit"])
    tok = _Tok(vocab_size=cfg.vocab_size, seg_token_idx=cfg.seg_token_idx)
    assert not m.decode_8bit
    w = MW.ModelWorker(m, tok, args)
    assert m.decode_8bit
    g = torch.Generator().manual_seed(2)
    image = torch.randint(0, 256, (90, 120, 3), generator=g, dtype=torch.uint8).numpy()
    prompt = "<im_start><image><im_end>\nWhat is shown here? Segment it."
    params = {"prompt": prompt, "images": [image], "temperature": 0.0, "max_new_tokens": 12}
    msgs = [json.loads(r[:-1].decode()) for r in w.generate_stream_gate(dict(params))]
    assert len(msgs) == 12 and all(x["error_code"] == 0 for x in msgs)
    clip, _, _, _ = w._images(params)
    ids = np.asarray([MW.tokenize_with_image_tokens(prompt, tok)], dtype=np.int64)
    new_ids = m.generate(ids, images=clip, max_new_tokens=12, eos_token_id=-1)[0, ids.shape[1]:].tolist()
    assert m.decode_8bit and msgs[-1]["text"] == prompt + tok.decode(new_ids)
