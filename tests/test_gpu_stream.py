"""MedPLIBForCausalLM.generate_stream (greedy and temperature sampling, token-by-token loop and captured graph) and the serving worker's face
over it, on the tiny config: dense, E = 2 top-1 and E = 2 top-2."""
import json

import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM
from toy_tokenizer import ToyTokenizer  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("dense", "top1", "top2")
N_NEW = 24
D = 1e-4                    # the band of tests/test_gpu_sample.py


def _cdf64(row, T):
    """(CDF normalised to 1, weights) of softmax(row / T) in float64."""
    l = row.astype(np.float64)
    w = np.exp((l - l.max()) / T)
    c = np.cumsum(w)
    return c / c[-1], w


def _tiny(dev, kind, **kw):
    from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM
    if kind == "dense":
        cfg, cls = MedPLIBConfig.tiny(moe_enable=False, sam_depth=2, **kw), LISAForCausalLM
    else:
        cfg, cls = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, num_experts=2, top_k_experts=1 if kind == "top1" else 2, **kw), MedPLIBForCausalLM
    W = OM.init_hf_weights(cfg, seed=3)
    m = cls(cfg, device=dev)
    m.load_hf_state_dict(W)
    return cfg, m.eval()


def _inputs(cfg, dev, seed=0):
    b = OM.make_batch(cfg, 1, seed=seed)
    return b, b["images_clip"].to(torch.bfloat16).to(dev), b["images"].to(torch.bfloat16).float().to(dev)


def _paths(m):
    return (True, False) if m._graph_decode_ok() else (False,)


def _stream(m, b, clip, graph, **kw):
    m.decode_with_graph = graph
    kw.setdefault("eos_token_id", -1)
    kw.setdefault("max_new_tokens", N_NEW)
    out = list(m.generate_stream(b["input_ids"], clip, **kw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_stream_equals_generate_and_evaluate(dev, kind):
    """temperature = 0: the last yield's ids are generate()'s new tokens, every yield is a prefix of the next, and with a generated token
    standing in for <SEG> and a later one for EOS the mask of the stopping yield is evaluate()'s, bit for bit; in the loop and in the graph."""
    cfg, m = _tiny(dev, kind)
    b, clip, sam = _inputs(cfg, dev)
    n_in = b["input_ids"].shape[1]
    for graph in _paths(m):
        m.decode_with_graph = graph
        ref = m.generate(b["input_ids"], images=clip, max_new_tokens=N_NEW, eos_token_id=-1)[0, n_in:].tolist()
        ys = _stream(m, b, clip, graph, temperature=0.0)
        assert m.last_decode_path == ("graph" if graph else "loop")
        assert len(ys) == N_NEW and ys[-1][0] == ref and not ys[-1][1]
        assert all(a[0] == bb[0][:len(a[0])] for a, bb in zip(ys, ys[1:]))
        assert all(y[2] is None for y in ys)                        # no SAM image given: no mask
        # a token the run emits stands in for <SEG>, a later one for EOS: the mask comes with the stopping yield and is evaluate()'s
        seg = ref[5]
        at = next(i for i in range(8, N_NEW) if ref[i] not in ref[:i])
        m.seg_token_idx = seg
        try:
            ids_e, masks_e = m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=N_NEW, eos_token_id=ref[at])
            kw = dict(temperature=0.0, images=sam, resize_list=b["resize_list"], original_size_list=b["label_list"])
            ys = _stream(m, b, clip, graph, eos_token_id=ref[at], **kw)
            assert len(ys) == at + 1 and ys[-1][1] and ys[-1][0] == ids_e[0, n_in:].tolist() == ref[:at + 1]
            assert all(y[2] is None for y in ys[:-1]) and torch.equal(ys[-1][2], masks_e[0])
            # an answer that runs into max_new_tokens is not a stop: no mask, as in the reference
            ys = _stream(m, b, clip, graph, **kw)
            assert len(ys) == N_NEW and not ys[-1][1] and seg in ys[-1][0] and all(y[2] is None for y in ys)
        finally:
            m.seg_token_idx = cfg.seg_token_idx


@pytest.mark.parametrize("kind", KINDS)
def test_sampling_stream(dev, kind):
    """temperature = 0.7: in each path every token is inside the float64 band of that step's own logits and u, u_i is gate_noise(1, seed, i),
    one seed gives one answer, and two seeds differ within 32 tokens on a distribution whose entropy is first checked to exceed 1 nat."""
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev, seed=1)
    T, seed = 0.7, 5
    for graph in _paths(m):
        dbg = []
        ys = _stream(m, b, clip, graph, temperature=T, sample_seed=seed, max_new_tokens=32, debug=dbg)
        assert m.last_decode_path == ("graph" if graph else "loop")
        ids = ys[-1][0]
        assert len(dbg) == len(ids) == 32 and [t for _, _, t in dbg] == ids
        entropies = []
        for i, (row, u, t) in enumerate(dbg):
            assert u == float(ops.gate_noise(1, seed, i, False, dev)[0]), (graph, i)
            cdf, w = _cdf64(row.numpy(), T)
            lo = cdf[t - 1] if t > 0 else 0.0
            assert w[t] > 0 and lo - D <= u <= cdf[t] + D, (graph, i, t, u, lo, cdf[t])
            p = w / w.sum()
            entropies.append(float(-(p[p > 0] * np.log(p[p > 0])).sum()))
        assert min(entropies) > 1.0, min(entropies)                 # the seeds below cannot agree by default
        again = _stream(m, b, clip, graph, temperature=T, sample_seed=seed, max_new_tokens=32)
        assert again[-1][0] == ids
        other = _stream(m, b, clip, graph, temperature=T, sample_seed=seed + 1, max_new_tokens=32)
        assert other[-1][0] != ids


def test_injected_uniforms_force_the_loop(dev):
    cfg, m = _tiny(dev, "top1")
    b, clip, _ = _inputs(cfg, dev)
    us = np.random.default_rng(3).random(16)
    dbg = []
    ys = _stream(m, b, clip, True, temperature=0.7, max_new_tokens=16, uniforms=lambda i: us[i], debug=dbg)
    assert m.last_decode_path == "loop" and len(ys) == 16
    assert [u for _, u, _ in dbg] == [float(np.float32(x)) for x in us]
    for row, u, t in dbg:
        cdf, w = _cdf64(row.numpy(), 0.7)
        assert w[t] > 0 and (cdf[t - 1] if t > 0 else 0.0) - D <= u <= cdf[t] + D


@pytest.mark.parametrize("kind", ("dense", "top2"))
def test_yields_and_stop(dev, kind):
    """stream_interval = 3: yields after tokens 0, 3, 6, ... and the last one; a stop_token_id the greedy run emits ends the stream there."""
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev)
    for graph in _paths(m):
        full = _stream(m, b, clip, graph, temperature=0.0, max_new_tokens=20)[-1][0]
        ys = _stream(m, b, clip, graph, temperature=0.0, max_new_tokens=20, stream_interval=3)
        assert [len(y[0]) - 1 for y in ys] == [0, 3, 6, 9, 12, 15, 18, 19]
        assert all(y[0] == full[:len(y[0])] for y in ys) and not any(y[1] for y in ys)
        stop = next(t for i, t in enumerate(full) if i >= 4 and t not in full[:i])       # first emitted at step >= 4
        at = full.index(stop)
        ys = _stream(m, b, clip, graph, temperature=0.0, max_new_tokens=20, stream_interval=3, stop_token_id=stop)
        assert [len(y[0]) - 1 for y in ys] == sorted(set(list(range(0, at, 3)) + [at])) and ys[-1][0] == full[:at + 1]
        assert ys[-1][1] and not any(y[1] for y in ys[:-1])
        gate_pass = m.model.llm.gate_pass
        _stream(m, b, clip, graph, temperature=0.0, max_new_tokens=20, stream_interval=3, stop_token_id=stop)
        assert m.model.llm.gate_pass - gate_pass == at + 1             # prefill + one pass per fed token: replays past the stop are discarded


@pytest.mark.parametrize("short", ("cache", "table"))
@pytest.mark.parametrize("temperature", (0.0, 0.7))
def test_running_past_the_cache_or_the_rope_table_raises(dev, short, temperature):
    """A KV cache, or a RoPE table, 6 rows short of the request — sizes only: the bounded kernels read and write nothing past either.  The
    graph path raises through the error word (MP_POS_ERR_CACHE = 2, MP_POS_ERR_TABLE = 1) at the first look after the overrun, the yields
    before it having been delivered.  The token-by-token loop never reaches the device with such a position: LlamaStack.forward refuses a
    step that does not fit the cache on the host, and regrows a short table (the stream then completes)."""
    cfg, m = _tiny(dev, "top1")
    b, clip, _ = _inputs(cfg, dev)
    llm = m.model.llm
    make, tables = llm.new_kv_cache, (llm.cos, llm.sin, llm.sin_neg)

    def short_cache(batch, rows):
        return make(batch, rows - 6)

    def short_table(batch, rows):               # the cache as asked for, the tables cut to rows - 6 positions (prefix views: nothing is freed)
        cache = make(batch, rows)
        llm.cos, llm.sin = llm.cos[:rows - 6], llm.sin[:rows - 6]
        if llm.sin_neg is not None:
            llm.sin_neg = llm.sin_neg[:rows - 6]
        return cache

    kw = dict(temperature=temperature, max_new_tokens=16, stream_interval=4)
    try:
        llm.new_kv_cache = short_cache if short == "cache" else short_table
        seen = []
        with pytest.raises(RuntimeError, match="error word %d" % (2 if short == "cache" else 1)):
            m.decode_with_graph = True
            for y in m.generate_stream(b["input_ids"], clip, eos_token_id=-1, **kw):
                seen.append(len(y[0]))
        assert m.last_decode_path == "graph" and seen == [1, 5, 9]          # the token fed at step 11 is the first without a row
        llm.cos, llm.sin, llm.sin_neg = tables
        if short == "cache":
            with pytest.raises(ValueError, match="do not fit the KV cache"):
                _stream(m, b, clip, False, **kw)
        else:
            assert len(_stream(m, b, clip, False, **kw)) == 5
        assert m.last_decode_path == "loop"
    finally:
        llm.new_kv_cache = make
        llm.cos, llm.sin, llm.sin_neg = tables
    assert len(_stream(m, b, clip, True, **kw)) == 5


def test_generate_still_refuses_sampling_and_beams(dev):
    cfg, m = _tiny(dev, "dense")
    b, clip, _ = _inputs(cfg, dev)
    with pytest.raises(NotImplementedError):
        m.generate(b["input_ids"], images=clip, do_sample=True, temperature=0.7, max_new_tokens=4)
    with pytest.raises(NotImplementedError):
        m.generate(b["input_ids"], images=clip, num_beams=4, max_new_tokens=4)


class _Tok(ToyTokenizer):
    """The toy tokenizer with a decode: every ordinary id is the piece ' t<id>.', special ids decode to nothing."""

    def decode(self, ids, skip_special_tokens=True):
        special = set(self.special_ids.values()) | {self.bos_token_id, self.eos_token_id, self.pad_token_id}
        return "".join(f" t{i}." for i in ids if not (skip_special_tokens and i in special))


def test_worker_face(dev):
    from model.serve import model_worker as MW
    cfg, m = _tiny(dev, "top1")
    args = MW.parse_args(["--model-path", "checkpoints/tiny", "--device_map", "cuda", "--stream-interval", "2"])
    g = torch.Generator().manual_seed(2)
    image = torch.randint(0, 256, (90, 120, 3), generator=g, dtype=torch.uint8).numpy()
    prompt = "<im_start><image><im_end>\nWhat is shown here? Segment it."
    params = {"prompt": prompt, "images": [image], "temperature": 0.0, "max_new_tokens": 12}

    def run(tok, **extra):
        w = MW.ModelWorker(m, tok, args)
        raw = list(w.generate_stream_gate(dict(params, **extra)))
        assert all(r.endswith(b"\0") and r.count(b"\0") == 1 for r in raw)
        msgs = [json.loads(r[:-1].decode()) for r in raw]
        assert all(sorted(x) == ["error_code", "height", "mask", "text", "width"] and x["error_code"] == 0 for x in msgs)
        return w, msgs

    tok = _Tok(vocab_size=cfg.vocab_size, seg_token_idx=cfg.seg_token_idx)
    w, msgs = run(tok)
    assert len(msgs) == 7                                           # tokens 0, 2, 4, 6, 8, 10 and the last one (11)
    assert all(x["mask"] == [] and x["height"] == "0" and x["width"] == "0" for x in msgs)
    clip, sam, resize_list, sizes = w._images(params)
    ids = np.asarray([MW.tokenize_with_image_tokens(prompt, tok)], dtype=np.int64)
    new_ids = m.generate(ids, images=clip, max_new_tokens=12, eos_token_id=-1)[0, ids.shape[1]:].tolist()
    texts = [x["text"] for x in msgs]
    assert texts == [prompt + tok.decode(new_ids[:n]) for n in (1, 3, 5, 7, 9, 11, 12)]      # the text grows by the newly decoded tokens
    assert len(set(texts)) == 7
    # a token the answer holds stands in for <SEG>, a later one for </s> (the prompt keeps its ids): the stop ends the stream and its
    # message carries evaluate()'s thresholded mask
    seg = new_ids[3]
    at = next(i for i in range(5, 12) if new_ids[i] not in new_ids[:i])
    m.seg_token_idx = seg
    tok.special_ids["<SEG>"] = seg
    try:
        tok.eos_token_id = new_ids[at]
        w, msgs = run(tok)
        assert len(msgs) == len(set(range(0, at, 2)) | {at})
        _, masks = m.evaluate(clip, sam, ids, resize_list, sizes, max_new_tokens=12, eos_token_id=new_ids[at])
        ref = (torch.sigmoid(masks[0].float()) > 0.1).int().squeeze(0).cpu().numpy()
        last = msgs[-1]
        assert (last["height"], last["width"]) == ("90", "120") and last["mask"] == np.transpose(np.nonzero(ref)).tolist()
        assert all(x["mask"] == [] and x["height"] == "0" for x in msgs[:-1])
        assert last["text"] == prompt + tok.decode(new_ids[:at + 1])
        del tok.eos_token_id                                         # (back to the class's 2)
        # without a stop the answer runs into max_new_tokens: no mask, as in the reference
        _, msgs = run(tok)
        assert len(msgs) == 7 and all(x["mask"] == [] for x in msgs)
        # a stop string: the stream ends at the first message whose text holds it, the text cut at its last occurrence, the mask built
        stop = f" t{new_ids[at]}."
        _, cut = run(tok, stop=stop)
        assert len(cut) == len(range(0, at, 2)) + 1                  # the messages before it and the one (token at, or at + 1) that sees it
        seen = tok.decode(new_ids[:at + 1 if (at % 2 == 0 or at == 11) else at + 2])
        assert cut[-1]["text"] == prompt + seen[:seen.rfind(stop)] and cut[-1]["height"] == "90"
        assert all(x["mask"] == [] for x in cut[:-1])
    finally:
        m.seg_token_idx = cfg.seg_token_idx
