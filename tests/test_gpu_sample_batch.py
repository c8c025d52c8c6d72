"""Several sampled requests as the rows of one decode step: generate_sample_batch(), generate_stream_batch() and the worker's batch loop over
them, on the tiny config (dense, E = 2 top-1, E = 2 top-2), in the captured graph and in the token-by-token loop.  A row of a batch is the
single-prompt model in another summation order (tests/test_gpu_generate_batch.py), so no test compares the TOKENS of a batch row with the
single-prompt path; what is exact is checked exactly: every token is the single-row op on that step's own recorded logits row at the keyed
draw of its request."""
import json

import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd.model import generation as G
from oracle import model as OM
from sample_filter_cases import Row64
from test_gpu_generate_batch import KINDS, LENGTHS, _padded, _prompts, _tiny
from test_gpu_stream import _paths, _Tok

pytestmark = pytest.mark.gpu

N_NEW = 16
ROW_PARAMS = ((0.7, 5, 0.9), (1.3, 0, 1.0), (0.2, 50, 0.9))      # (temperature, top_k, top_p) of the three rows


def _single_row_op(row, u, T, k, p, dev):
    """generate_sample()'s pick on one recorded logits row [V] at the draw u."""
    logits, u = row.to(dev).view(1, -1), torch.tensor([u], dtype=torch.float32, device=dev)
    if k == 0 and p >= 1.0:
        return int(ops.sample_rows(logits, u, T)[0])
    return int(ops.sample_rows_filtered(logits, u, T, k, p)[0])


def _sample(m, cfg, dev, graph, seed, debug=None, n_new=N_NEW, params=ROW_PARAMS, **kw):
    p = _prompts(cfg, dev)
    ids, clip, att = _padded(p)
    m.decode_with_graph = graph
    out = m.generate_sample_batch(ids, images=clip, attention_mask=att, max_new_tokens=n_new, eos_token_id=-1, temperature=[q[0] for q in params],
                                  top_k=[q[1] for q in params], top_p=[q[2] for q in params], sample_seed=seed, debug=debug, **kw)
    torch.cuda.synchronize()
    assert m.last_decode_path == ("graph" if graph else "loop")
    return out


@pytest.mark.parametrize("kind,mode", [(k, "bf16") for k in KINDS] + [(k, q) for k in ("dense", "top1") for q in ("w8", "w4")])
def test_every_token_is_the_single_row_op_on_its_own_logits(dev, kind, mode):
    cfg, m = _tiny(dev, kind)
    if mode == "w8":
        m.enable_decode_8bit(True)
    elif mode == "w4":
        m.enable_decode_4bit(True)
    seed = 5
    for graph in _paths(m):
        dbg = []
        out = _sample(m, cfg, dev, graph, seed, debug=dbg)
        assert out.shape == (3, max(LENGTHS) + N_NEW) and len(dbg) == N_NEW
        entropies = []
        for i, (logits, u, toks) in enumerate(dbg):
            assert logits.shape == (3, cfg.vocab_size) and logits.dtype == torch.float32 and u.shape == (3,) and len(toks) == 3
            for b, (T, k, p) in enumerate(ROW_PARAMS):
                assert float(u[b]) == float(ops.gate_noise(1, seed + b, i, False, dev)[0]), (graph, i, b)
                assert toks[b] == _single_row_op(logits[b], float(u[b]), T, k, p, dev) == int(out[b, LENGTHS[b] + i]), (graph, i, b)
                r64 = Row64(logits[b].numpy(), T)
                cut, _ = r64.cut(k, p)
                pk = r64.w[r64.l >= cut] / r64.w[r64.l >= cut].sum()
                entropies.append(float(-(pk[pk > 0] * np.log(pk[pk > 0])).sum()))
        assert max(entropies) > 0.5, max(entropies)                # the seeds below cannot agree by default
        assert torch.equal(_sample(m, cfg, dev, graph, seed), out)
        assert not torch.equal(_sample(m, cfg, dev, graph, seed + 1), out)


@pytest.mark.parametrize("kind", KINDS)
def test_top_k_1_is_generate_batch_and_graph_equals_loop(dev, kind):
    cfg, m = _tiny(dev, kind)
    ids, clip, att = _padded(_prompts(cfg, dev))
    runs = []
    for graph in _paths(m):
        m.decode_with_graph = graph
        greedy = m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=N_NEW, eos_token_id=-1)
        cold = _sample(m, cfg, dev, graph, 3, params=((0.7, 1, 1.0), (1.3, 1, 0.9), (0.2, 1, 1.0)))
        assert torch.equal(cold, greedy), graph
        runs.append(_sample(m, cfg, dev, graph, 8))
    if len(runs) == 2:
        assert torch.equal(runs[0], runs[1])                        # token for token


def _requests(cfg, dev, lengths=LENGTHS, sam=(), **per_row):
    """One StreamRequest per length; per_row: name -> one value per request.  sam: the rows that carry a SAM image."""
    out = []
    for s, L in enumerate(lengths):
        b = OM.make_batch(cfg, 1, seed=s, L=L)
        kw = {k: v[s] for k, v in per_row.items()}
        if s in sam:
            kw.update(images=b["images"].to(torch.bfloat16).float().to(dev), resize_list=b["resize_list"], original_size_list=b["label_list"])
        out.append(G.StreamRequest(input_ids=np.asarray(b["input_ids"]).astype(np.int64), images_clip=b["images_clip"].to(torch.bfloat16).to(dev),
                                   **kw))
    return out


def _stream(m, requests, graph, **kw):
    """-> the yields per row."""
    m.decode_with_graph = graph
    kw.setdefault("eos_token_id", -1)
    rows = [[] for _ in requests]
    for row, ids, stopped, mask in m.generate_stream_batch(requests, **kw):
        rows[row].append((list(ids), stopped, mask))
    torch.cuda.synchronize()
    assert m.last_decode_path == ("graph" if graph else "loop")
    return rows


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_requests_share_one_step(dev, kind):
    """One greedy request, one sampled with apply_top_p, one sampled whose top_p and top_k are given but not applied."""
    cfg, m = _tiny(dev, kind)
    T = 0.7
    reqs = _requests(cfg, dev, temperature=(0.0, T, T), top_p=(0.5, 0.9, 0.1), top_k=(3, 5, 1), apply_top_p=(False, True, False),
                     sample_seed=(11, 12, 13), max_new_tokens=(N_NEW,) * 3)
    for graph in _paths(m):
        dbg = []
        ys = _stream(m, reqs, graph, debug=dbg)
        assert len(dbg) == N_NEW and [len(y) for y in ys] == [N_NEW] * 3
        for i, (logits, u, toks) in enumerate(dbg):
            assert toks[0] == int(torch.argmax(logits[0]))
            assert float(u[1]) == float(ops.gate_noise(1, 12, i, False, dev)[0]) and float(u[2]) == float(ops.gate_noise(1, 13, i, False, dev)[0])
            assert toks[1] == _single_row_op(logits[1], float(u[1]), T, 5, 0.9, dev)
            assert toks[2] == _single_row_op(logits[2], float(u[2]), T, 0, 1.0, dev)          # top_p = 0.1 and top_k = 1 are ignored
            assert [y[-1][0][i] for y in ys] == list(toks)
        assert len({tuple(y[-1][0]) for y in ys}) == 3


@pytest.mark.parametrize("kind", ("dense", "top1"))
def test_rows_yield_and_stop_on_their_own(dev, kind):
    cfg, m = _tiny(dev, kind)
    limits = (5, 12, 9)
    kw = dict(temperature=(0.0, 0.7, 1.3), sample_seed=(1, 2, 3), max_new_tokens=limits)
    for graph in _paths(m):
        free = [y[-1][0] for y in _stream(m, _requests(cfg, dev, **kw), graph)]
        assert [len(a) for a in free] == list(limits)
        # a stop id that row 1 emits (not before its fourth token) and the others never do
        at, stop = next((i, t) for i, t in enumerate(free[1]) if i >= 3 and t not in free[1][:i] and t not in free[0] and t not in free[2])
        ys = _stream(m, _requests(cfg, dev, **kw), graph, stream_interval=2, eos_token_id=stop)
        assert [len(y[0]) - 1 for y in ys[0]] == [0, 2, 4] and [len(y[0]) - 1 for y in ys[2]] == [0, 2, 4, 6, 8]
        assert [len(y[0]) - 1 for y in ys[1]] == sorted(set(range(0, at, 2)) | {at})
        for r in range(3):
            assert all(a[0] == b[0][:len(a[0])] for a, b in zip(ys[r], ys[r][1:]))
            assert not any(y[1] for y in ys[r][:-1]) and all(y[2] is None for y in ys[r])
        assert ys[1][-1][1] and ys[1][-1][0] == free[1][:at + 1]
        assert not ys[0][-1][1] and ys[0][-1][0] == free[0] and not ys[2][-1][1] and ys[2][-1][0] == free[2]
        every = _stream(m, _requests(cfg, dev, **kw), graph, stream_interval=1, eos_token_id=stop)
        assert [y[-1][0] for y in every] == [y[-1][0] for y in ys]
        assert [len(y) for y in every] == [5, at + 1, 9]
        # a stop_check on row 2 alone: true at its third yield (five ids), which stops that row only
        checked = _requests(cfg, dev, stop_check=(None, None, lambda ids: len(ids) >= 4), **kw)
        ys = _stream(m, checked, graph, stream_interval=2)
        assert [len(y[0]) for y in ys[2]] == [1, 3, 5] and ys[2][-1][1] and ys[2][-1][0] == free[2][:5]
        assert ys[0][-1][0] == free[0] and ys[1][-1][0] == free[1] and not ys[0][-1][1] and not ys[1][-1][1]
        # the per-request stop id
        own = _requests(cfg, dev, stop_token_id=(None, stop, None), **kw)
        ys = _stream(m, own, graph, stream_interval=2)
        assert ys[1][-1][1] and ys[1][-1][0] == free[1][:at + 1] and [y[-1][0] for y in (ys[0], ys[2])] == [free[0], free[2]]


@pytest.mark.parametrize("kind", ("dense", "top2"))
def test_the_stopping_yield_carries_the_rows_own_mask(dev, kind):
    """A token row 0 emits stands in for <SEG> and a later one for eos: its stopping yield carries _seg_mask on its own ids and hidden states.
    Row 1 has a SAM image too but runs into its limit: no mask.  Row 2 stops by its own stop id and has no SAM image: no mask."""
    cfg, m = _tiny(dev, kind)
    n = 12
    kw = dict(temperature=(0.0,) * 3, max_new_tokens=(n,) * 3)
    for graph in _paths(m):
        free = [y[-1][0] for y in _stream(m, _requests(cfg, dev, **kw), graph)]
        seg = free[0][2]
        at, eos = next((i, t) for i, t in enumerate(free[0]) if i >= 4 and t not in free[0][:i] and t not in free[1] and t not in free[2])
        at2 = max(free[2].index(t) for t in set(free[2]))            # the latest first occurrence of a token in row 2's answer
        stop2 = free[2][at2]
        reqs = _requests(cfg, dev, sam=(0, 1), stop_token_id=(None, None, stop2), **kw)
        m.seg_token_idx = seg
        try:
            ys = _stream(m, reqs, graph, eos_token_id=eos)
            assert ys[0][-1][1] and ys[0][-1][0] == free[0][:at + 1] and seg in ys[0][-1][0]
            assert ys[2][-1][1] and ys[2][-1][0] == free[2][:at2 + 1] and not ys[1][-1][1] and len(ys[1][-1][0]) == n
            assert all(y[2] is None for r in range(3) for y in ys[r][:-1]) and ys[1][-1][2] is None and ys[2][-1][2] is None
            # the row's own ids and hidden states, from the batch driver itself
            prompts = [(r.input_ids, r.images_clip, G.NO_EXTRAS) for r in reqs]
            with m._decoding("test"):
                for generated, _, hiddens in m._decode_batch(prompts, n, (eos,)):
                    pass
                assert list(generated[0]) == free[0][:at + 1]
                output_ids = np.concatenate([reqs[0].input_ids, np.asarray(generated[0], dtype=np.int64)[None]], 1)
                want = m._seg_mask(output_ids, list(hiddens[0]), reqs[0].images, reqs[0].resize_list, reqs[0].original_size_list)[0]
            assert ys[0][-1][2] is not None and torch.equal(ys[0][-1][2], want)
        finally:
            m.seg_token_idx = cfg.seg_token_idx


def test_refusals_leave_the_model_decoding_as_before(dev):
    def unchanged(m, cfg, call, error, match):
        ids, clip, att = _padded(_prompts(cfg, dev))
        before = m.generate(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
        pass0, training = m.model.llm.gate_pass, m.training
        with pytest.raises(error, match=match):
            call(ids, clip, att)
        assert m.model.llm.gate_pass == pass0 and m.training == training
        assert torch.equal(m.generate(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1), before)

    def sample(**kw):
        return lambda ids, clip, att: m.generate_sample_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1, **kw)

    def stream(n):
        return lambda ids, clip, att: list(m.generate_stream_batch(_requests(cfg, dev, (24,) * n)))

    cfg, m = _tiny(dev, "top1")
    llm = m.model.llm
    unchanged(m, cfg, stream(9), ValueError, "1 to 8")
    unchanged(m, cfg, stream(0), ValueError, "1 to 8")
    unchanged(m, cfg, sample(temperature=0), ValueError, "strictly positive")
    unchanged(m, cfg, sample(temperature=[0.7, 0.0, 1.0]), ValueError, "strictly positive")
    unchanged(m, cfg, sample(temperature=[0.7, 1.0]), ValueError, "one per row")
    unchanged(m, cfg, sample(top_p=[0.9] * 4), ValueError, "one per row")
    unchanged(m, cfg, sample(do_sample=False), ValueError, "generate_batch")
    unchanged(m, cfg, sample(batch_rows=9), ValueError, "1..8")
    unchanged(m, cfg, sample(num_beams=2), NotImplementedError, "generate_beam")
    unchanged(m, cfg, lambda ids, clip, att: m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, do_sample=True),
              NotImplementedError, "generate_sample")
    llm.cfg.moe_gate_sampling = True                 # (its draws are keyed on the pass number: only the refusals themselves are checked)
    pass0 = llm.gate_pass
    ids, clip, att = _padded(_prompts(cfg, dev))
    with pytest.raises(NotImplementedError, match="moe_gate_sampling"):
        m.generate_sample_batch(ids, images=clip, attention_mask=att, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match="moe_gate_sampling"):
        m.generate_stream_batch(_requests(cfg, dev))             # (refused at the call, not at the first next())
    assert llm.gate_pass == pass0 and not m.training
    cfg, m = _tiny(dev, "top1", use_residual=True)
    unchanged(m, cfg, sample(), NotImplementedError, "use_residual")
    unchanged(m, cfg, stream(3), NotImplementedError, "use_residual")


def _worker_messages(raw, n):
    """[(index, bytes)] -> the decoded messages per index, each checked for the wire format."""
    per = [[] for _ in range(n)]
    for index, r in raw:
        assert r.endswith(b"\0") and r.count(b"\0") == 1
        x = json.loads(r[:-1].decode())
        assert sorted(x) == ["error_code", "height", "mask", "text", "width"] and x["error_code"] == 0
        per[index].append(x)
    return per


def test_worker_serves_a_list_of_requests(dev, monkeypatch):
    from model.serve import model_worker as MW
    cfg, m = _tiny(dev, "top1")
    base = ["--model-path", "checkpoints/tiny", "--device_map", "cuda", "--stream-interval", "2"]
    g = torch.Generator().manual_seed(2)
    image = torch.randint(0, 256, (90, 120, 3), generator=g, dtype=torch.uint8).numpy()
    prompt = "<im_start><image><im_end>\nWhat is shown here? Segment it."
    tok = _Tok(vocab_size=cfg.vocab_size, seg_token_idx=cfg.seg_token_idx)
    tok.eos_token_id = -1
    limits = (12, 7, 9)
    params = [{"prompt": prompt + " " * i, "images": [image], "temperature": t, "max_new_tokens": n} for i, (t, n) in enumerate(zip((0.0, 0.7, 1.3), limits))]
    sizes = []
    batch = m.generate_stream_batch
    monkeypatch.setattr(m, "generate_stream_batch", lambda reqs, **kw: (sizes.append(len(reqs)), batch(reqs, **kw))[1])

    def run(flags, seed, model=m, plist=params):
        torch.manual_seed(seed)                                     # every request's sampling seed comes from torch's generator, in list order
        w = MW.ModelWorker(model, tok, MW.parse_args(base + flags))
        per = _worker_messages(list(w.generate_stream_gate_batch(plist)), len(plist))
        for i, msgs in enumerate(per):
            texts = [x["text"] for x in msgs]
            assert texts[0].startswith(plist[i]["prompt"]) and all(b_.startswith(a_) for a_, b_ in zip(texts, texts[1:]))
        return per

    per = run([], 9)
    assert sizes == [3]
    assert [len(msgs) for msgs in per] == [len(set(range(0, n, 2)) | {n - 1}) for n in limits]
    assert all(x["mask"] == [] and x["height"] == "0" for msgs in per for x in msgs)
    assert run([], 9) == per and run([], 10) != per                # repeatable under torch.manual_seed
    # a stop string request 0 meets: its last message has the text cut at it, the others run to their limits
    pieces = per[0][-1]["text"][len(params[0]["prompt"]):].split(".")[:-1]
    stop = next(p for i, p in enumerate(pieces) if i >= 3 and p not in pieces[:i]) + "."
    cut = run([], 9, plist=[dict(params[0], stop=stop)] + params[1:])
    assert len(cut[0]) < len(per[0]) and cut[0][-1]["text"] == params[0]["prompt"] + "".join(p + "." for p in pieces[:pieces.index(stop[:-1])])
    assert cut[1:] == per[1:]
    # --limit-model-concurrency 2: groups of two and one
    del sizes[:]
    two = run(["--limit-model-concurrency", "2"], 9)
    assert sizes == [2, 1] and [len(msgs) for msgs in two] == [len(msgs) for msgs in per]
    # a model that refuses batch rows is served one request after the other, through the same generator: generate_stream's messages
    cfg_r, m_r = _tiny(dev, "top1", use_residual=True)
    assert m_r.model.llm.batch_rows_unsupported() is not None
    one_by_one = run([], 9, model=m_r)
    torch.manual_seed(9)
    w = MW.ModelWorker(m_r, tok, MW.parse_args(base))
    alone = [[json.loads(r[:-1].decode()) for r in w.generate_stream_gate(p)] for p in params]
    assert one_by_one == alone and [len(msgs) for msgs in alone] == [len(msgs) for msgs in per]
