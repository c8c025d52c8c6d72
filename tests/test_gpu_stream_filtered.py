"""Top-k / top-p sampling through the host layers, on the tiny config of tests/test_gpu_stream.py (dense, E = 2 top-1, E = 2 top-2), in the
token-by-token loop and in the captured graph: generate_stream(apply_top_p=True), generate_sample and the worker's --apply-top-p."""
import json

import numpy as np
import pytest
import torch

from medplib_amd import ops
from oracle import model as OM
from sample_filter_cases import Row64
from test_gpu_stream import D, KINDS, _inputs, _paths, _stream, _tiny, _Tok

pytestmark = pytest.mark.gpu

T, K, P = 0.7, 5, 0.9


@pytest.mark.parametrize("kind", KINDS)
def test_filtered_sampling_stream(dev, kind):
    """Every token is ops.sample_rows_filtered on that step's recorded logits and u, and lies in the float64 kept set widened by d (its logit
    is among the top k, and A(l) / Z > 1 - p - d); u_i is the keyed draw for (seed, i); one seed gives one answer and two seeds differ, on
    kept distributions whose entropy is first checked to exceed 0.5 nat at some step."""
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev, seed=1)
    seed = 5
    kw = dict(temperature=T, top_k=K, top_p=P, apply_top_p=True, max_new_tokens=32)
    for graph in _paths(m):
        dbg = []
        ys = _stream(m, b, clip, graph, sample_seed=seed, debug=dbg, **kw)
        assert m.last_decode_path == ("graph" if graph else "loop")
        ids = ys[-1][0]
        assert len(dbg) == len(ids) == 32 and [t for _, _, t in dbg] == ids
        entropies = []
        for i, (row, u, t) in enumerate(dbg):
            assert u == float(ops.gate_noise(1, seed, i, False, dev)[0]), (graph, i)
            again = ops.sample_rows_filtered(row.to(dev).view(1, -1), torch.tensor([u], dtype=torch.float32, device=dev), T, K, P)
            assert int(again[0]) == t, (graph, i, t, int(again[0]))
            r64 = Row64(row.numpy(), T)
            cut, t_k = r64.cut(K, P)
            l_t = float(row[t])
            assert l_t >= t_k and r64.ratio(l_t, t_k) > 1.0 - P - D, (graph, i, t, l_t, t_k)
            pk = r64.w[r64.l >= cut] / r64.w[r64.l >= cut].sum()
            entropies.append(float(-(pk[pk > 0] * np.log(pk[pk > 0])).sum()))
        assert max(entropies) > 0.5, max(entropies)                 # the seeds below cannot agree by default
        assert _stream(m, b, clip, graph, sample_seed=seed, **kw)[-1][0] == ids
        assert _stream(m, b, clip, graph, sample_seed=seed + 1, **kw)[-1][0] != ids


@pytest.mark.parametrize("kind", ("dense", "top2"))
def test_top_p_stays_ignored_without_apply_top_p(dev, kind):
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev, seed=1)
    for graph in _paths(m):
        ref = _stream(m, b, clip, graph, temperature=T, top_p=1.0, sample_seed=7, max_new_tokens=32)[-1][0]
        assert _stream(m, b, clip, graph, temperature=T, top_p=0.1, top_k=1, sample_seed=7, max_new_tokens=32)[-1][0] == ref
        assert _stream(m, b, clip, graph, temperature=T, top_p=0.1, sample_seed=7, max_new_tokens=32, apply_top_p=True)[-1][0] != ref


@pytest.mark.parametrize("kind", KINDS)
def test_top_k_1_is_greedy_through_the_whole_stack(dev, kind):
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev)
    n_in = b["input_ids"].shape[1]
    for graph in _paths(m):
        m.decode_with_graph = graph
        ref = m.generate(b["input_ids"], images=clip, max_new_tokens=32, eos_token_id=-1)[0, n_in:].tolist()
        ys = _stream(m, b, clip, graph, temperature=T, top_k=1, top_p=1.0, apply_top_p=True, sample_seed=3, max_new_tokens=32)
        assert m.last_decode_path == ("graph" if graph else "loop") and ys[-1][0] == ref


def test_generate_sample(dev):
    """Two ragged prompt rows: generate()'s layout (prompt included, right-padded with eos), repeatable under torch.manual_seed and under
    sample_seed, row b drawn under seed + b; top_k = 1 is generate(); temperature <= 0 and beams are refused."""
    cfg, m = _tiny(dev, "top1")
    b = OM.make_batch(cfg, 2, ragged=True)
    ids, att = b["input_ids"], b["attention_mask"]
    clip = b["images_clip"].to(dev).to(torch.bfloat16)
    lens = [int(att[r].sum()) for r in range(2)]
    assert lens[0] != lens[1]
    N, eos = 12, -1
    kw = dict(images=clip, attention_mask=att, max_new_tokens=N, eos_token_id=eos)
    for graph in _paths(m):
        m.decode_with_graph = graph
        torch.manual_seed(11)
        a = m.generate_sample(ids, temperature=T, top_k=K, top_p=P, **kw)
        assert m.last_decode_path == ("graph" if graph else "loop")
        torch.manual_seed(11)
        assert torch.equal(m.generate_sample(ids, temperature=T, top_k=K, top_p=P, **kw), a)
        assert a.shape == (2, max(lens) + N) and a.dtype == torch.int64
        for r in range(2):
            assert torch.equal(a[r, :lens[r]], torch.as_tensor(ids)[r, :lens[r]]) and (a[r, lens[r] + N:] == eos).all()
        s = m.generate_sample(ids, temperature=T, top_k=K, top_p=P, sample_seed=40, **kw)
        assert torch.equal(m.generate_sample(ids, temperature=T, top_k=K, top_p=None, sample_seed=40, **kw),
                           m.generate_sample(ids, temperature=T, top_k=K, top_p=1.0, sample_seed=40, **kw))
        # row 1 alone under seed 41 is row 1 of the batch under seed 40
        one = m.generate_sample(ids[1:2], images=clip[1:2], attention_mask=att[1:2], max_new_tokens=N, eos_token_id=eos, temperature=T, top_k=K,
                                top_p=P, sample_seed=41)
        assert torch.equal(one[0], s[1, :lens[1] + N])
        greedy = m.generate(ids, **kw)
        assert torch.equal(m.generate_sample(ids, temperature=T, top_k=1, **kw), greedy)
        assert torch.equal(m.generate_sample(ids, temperature=0.2, top_k=0, top_p=0.0, do_sample=True, num_beams=1, use_cache=True, **kw), greedy)
    for bad in (0, 0.0, -1.0):
        with pytest.raises(ValueError, match="strictly positive"):
            m.generate_sample(ids, temperature=bad, **kw)
    with pytest.raises(NotImplementedError, match="beam"):
        m.generate_sample(ids, num_beams=4, **kw)
    with pytest.raises(NotImplementedError, match="generate_sample"):
        m.generate(ids, do_sample=True, temperature=T, **kw)


def test_worker_applies_top_p_only_when_asked(dev):
    from model.serve import model_worker as MW
    cfg, m = _tiny(dev, "top1")
    base = ["--model-path", "checkpoints/tiny", "--device_map", "cuda", "--stream-interval", "2"]
    g = torch.Generator().manual_seed(2)
    image = torch.randint(0, 256, (90, 120, 3), generator=g, dtype=torch.uint8).numpy()
    prompt = "<im_start><image><im_end>\nWhat is shown here? Segment it."
    tok = _Tok(vocab_size=cfg.vocab_size, seg_token_idx=cfg.seg_token_idx)
    tok.eos_token_id = -1

    def run(flags, seed, **extra):
        torch.manual_seed(seed)                                     # the worker takes every request's sampling seed from torch's generator
        w = MW.ModelWorker(m, tok, MW.parse_args(base + flags))
        raw = list(w.generate_stream_gate(dict({"prompt": prompt, "images": [image], "temperature": T, "max_new_tokens": 12}, **extra)))
        msgs = [json.loads(r[:-1].decode()) for r in raw]
        assert all(r.endswith(b"\0") for r in raw) and all(x["error_code"] == 0 for x in msgs)
        texts = [x["text"] for x in msgs]
        assert len(texts) == 7 and all(b_.startswith(a_) for a_, b_ in zip(texts, texts[1:])) and texts[0].startswith(prompt)
        return texts

    today = run([], 9)
    assert run([], 9, top_p=0.05, top_k=1) == today                 # without the flag the request's top_p (and top_k) change nothing
    assert run(["--apply-top-p"], 9, top_p=1.0) == today            # the flag with nothing to truncate: the plain pick
    cold = run(["--apply-top-p"], 9, top_p=0.0)
    assert cold == run(["--apply-top-p"], 10, top_p=0.0) == run(["--apply-top-p"], 9, top_k=1) == run([], 9, temperature=0.0)    # the argmax
    assert cold != today
