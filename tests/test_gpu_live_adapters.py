"""Decoding with LoRA adapters attached (MedPLIBForCausalLM.adapters_merged: a non-destructive shadow merge, LoRAState.merge_shadow /
restore_plain over mp_lora_merge_rows_batched) on the tiny config: evaluate() / generate() / generate_stream() compute what a twin model
computes after merge_and_unload(), bit for bit and with the launches of the adapter-less model, and leave the weights, the adapters and the
training state as they found them.

Adapter values are dyadic (A in {-4..4} 2^-8, B in {-4..4} 2^-6, scaling 2): B A is exact in fp32 in any order, so the torch merge of the
twin (LoRAState.merge_into) and the kernel must produce the same bf16 weights (tests/test_gpu_lora_merge.py), hence the same tokens, hidden
states and masks."""
import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM
from test_gpu_launch_trace import _traced

pytestmark = pytest.mark.gpu

N_NEW = 10
ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
SPECS = {
    "dense-all7-r16": dict(moe=False, r=16, alpha=32, targets=ALL7),
    "top1-e2-qv-mlp-r8": dict(moe=True, E=2, k=1, r=8, alpha=16, targets="q_proj,v_proj,gate_proj,up_proj,down_proj"),
    "top2-e4-mlp-r8": dict(moe=True, E=4, k=2, r=8, alpha=16, targets="gate_proj,up_proj,down_proj"),
}
WEIGHT_KEYS = ("qkv", "o", "gu", "down", "qkv_rope")


def _build(dev, spec, adapters=True, dropout=0.0, layers=2):
    from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM
    if spec["moe"]:
        cfg = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, num_hidden_layers=layers, num_experts=spec["E"], top_k_experts=spec["k"])
        cls = MedPLIBForCausalLM
    else:
        cfg, cls = MedPLIBConfig.tiny(moe_enable=False, sam_depth=2, num_hidden_layers=layers), LISAForCausalLM
    m = cls(cfg, device=dev)
    m.load_hf_state_dict(OM.init_hf_weights(cfg, seed=3))
    if adapters:
        m.enable_lora(lora_r=spec["r"], lora_alpha=spec["alpha"], lora_dropout=dropout, lora_target_modules=spec["targets"])
    return cfg, m.eval()


def _set_adapters(m, dev, zero_b=False, seed=17):
    g = torch.Generator().manual_seed(seed)
    lora = m.model.lora
    assert abs(lora.scaling - 2.0) == 0
    for n, p in zip(lora.names, lora.params):
        if "lora_A" in n:
            p.data.copy_((torch.randint(-4, 5, p.shape, generator=g).float() * 2.0 ** -8).to(dev))
        elif "lora_B" in n:
            v = torch.randint(-4, 5, p.shape, generator=g).float() * 2.0 ** -6
            p.data.copy_((torch.zeros_like(v) if zero_b else v).to(dev))


def _inputs(cfg, dev):
    b = OM.make_batch(cfg, 1, seed=0)
    return b, b["images_clip"].to(torch.bfloat16).to(dev), b["images"].to(torch.bfloat16).float().to(dev)


def _capture_hidden(m):
    """Wrap m._decode so that the hidden states of the last yield (the prompt's and every fed token's) are kept: -> dict with "hidden"."""
    seen, orig = {}, type(m)._decode

    def wrapped(*a, **k):
        inner = orig(m, *a, **k)
        try:
            for generated, stopped, hiddens in inner:
                seen["hidden"] = torch.cat(list(hiddens), 1)
                yield generated, stopped, hiddens
        finally:
            inner.close()
    m._decode = wrapped
    return seen


def _run_all(m, inp, graph):
    """Every decode entry point once -> {name: tuple of host values}."""
    b, clip, sam = inp
    n_in = b["input_ids"].shape[1]
    seen = _capture_hidden(m)
    m.decode_with_graph = graph
    out = {}
    try:
        ids, masks = m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=N_NEW, eos_token_id=-1)
        assert m.last_decode_path == ("graph" if graph else "loop")
        out["evaluate"] = (ids.clone(), masks[0].float().cpu(), seen["hidden"].float().cpu())
        ids = m.generate(b["input_ids"], images=clip, max_new_tokens=N_NEW, eos_token_id=-1)
        out["generate"] = (ids.clone(), seen["hidden"].float().cpu())
        # a token the greedy run emits stands in for <SEG>; the stream stops itself after 8 tokens: the stopping yield carries the mask
        m.seg_token_idx = int(ids[0, n_in + 2])
        for T in (0.0, 0.7):
            ys = list(m.generate_stream(b["input_ids"], clip, images=sam, resize_list=b["resize_list"], original_size_list=b["label_list"],
                                        temperature=T, sample_seed=5, max_new_tokens=N_NEW, eos_token_id=-1, stop_check=lambda new: len(new) >= 8))
            assert ys[-1][1] and len(ys[-1][0]) == 8 and all(y[2] is None for y in ys[:-1])
            mask = ys[-1][2]
            if T == 0.0:
                assert mask is not None
            out[f"stream-T{T}"] = ([y[0] for y in ys], None if mask is None else mask.float().cpu(), seen["hidden"].float().cpu())
    finally:
        m.seg_token_idx = m.config.seg_token_idx
        del m._decode
    torch.cuda.synchronize()
    return out


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b


def _paths(m):
    return (True, False) if m._graph_decode_ok() else (False,)


_WORLDS = {}


def _world(dev, name):
    """Per model kind, built once: the live model (adapters attached), the adapter-less model, and what the merged twin and the adapter-less
    model decode on each path."""
    if name not in _WORLDS:
        spec = SPECS[name]
        cfg, live = _build(dev, spec)
        _set_adapters(live, dev)
        _, twin = _build(dev, spec)
        _set_adapters(twin, dev)
        twin.merge_and_unload()
        assert twin.model.lora is None
        _, base = _build(dev, spec, adapters=False)
        inp = _inputs(cfg, dev)
        w = dict(cfg=cfg, live=live, base=base, inp=inp, merged={g: _run_all(twin, inp, g) for g in _paths(twin)},
                 plain={g: _run_all(base, inp, g) for g in _paths(base)})
        del twin
        _WORLDS[name] = w
    return _WORLDS[name]


def _snapshot(m):
    llm = m.model.llm
    snap = {(i, k): lw[k].clone() for i, lw in enumerate(llm.layers) for k in WEIGHT_KEYS if k in lw}
    snap["lm_head"], snap["embed_tokens"] = llm.lm_head.clone(), llm.embed_tokens.clone()
    return snap, m.model.lora.step


def _assert_untouched(m, snap, what):
    weights, step = snap
    llm = m.model.llm
    for key, t in weights.items():
        now = getattr(llm, key) if isinstance(key, str) else llm.layers[key[0]][key[1]]
        assert torch.equal(now, t), f"{what}: {key} changed"
    assert m.model.lora is not None and m.model.llm.lora is m.model.lora, what
    assert m.model.lora.step == step and not m.model.lora.shadow_live and m._shadow_depth == 0, what


@pytest.mark.parametrize("name", list(SPECS))
def test_decode_with_adapters_equals_the_merged_twin(dev, name):
    """(on the parent commit: RuntimeError '... call merge_and_unload() first' from the first entry point)"""
    w = _world(dev, name)
    live = w["live"]
    assert set(_paths(live)) == set(w["merged"])
    for graph in _paths(live):
        got, want, plain = _run_all(live, w["inp"], graph), w["merged"][graph], w["plain"][graph]
        for entry in want:
            assert _equal(got[entry], want[entry]), f"{name}, graph={graph}: {entry}() differs from the merged twin"
        # the adapters act: the tokens differ from the adapter-less model's, or at least the hidden states do
        same_ids = _equal(got["evaluate"][0], plain["evaluate"][0])
        print(f"{name}, graph={graph}: ids {'equal' if same_ids else 'differ'} from the adapter-less model's")
        assert not same_ids or not torch.equal(got["evaluate"][2], plain["evaluate"][2])
        assert not torch.equal(got["evaluate"][2], plain["evaluate"][2])


@pytest.mark.parametrize("name", list(SPECS))
def test_fresh_adapters_decode_like_the_base_model(dev, name):
    """B = 0: bf16(W + 0) = W, so everything is bit-equal to the model without adapters."""
    w = _world(dev, name)
    _, fresh = _build(dev, SPECS[name])
    _set_adapters(fresh, dev, zero_b=True)
    for graph in _paths(fresh):
        got = _run_all(fresh, w["inp"], graph)
        for entry, want in w["plain"][graph].items():
            assert _equal(got[entry], want), f"{name}, graph={graph}: {entry}() differs from the adapter-less model"


@pytest.mark.parametrize("name", list(SPECS))
def test_nothing_is_left_behind(dev, name):
    w = _world(dev, name)
    m, (b, clip, sam) = w["live"], w["inp"]
    snap = _snapshot(m)
    m.decode_with_graph = _paths(m)[0]
    m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=N_NEW, eos_token_id=-1)
    _assert_untouched(m, snap, "evaluate")
    m.generate(b["input_ids"], images=clip, max_new_tokens=N_NEW, eos_token_id=-1)
    _assert_untouched(m, snap, "generate")
    list(m.generate_stream(b["input_ids"], clip, temperature=0.0, max_new_tokens=N_NEW, eos_token_id=-1))
    _assert_untouched(m, snap, "generate_stream")
    stream = m.generate_stream(b["input_ids"], clip, temperature=0.0, max_new_tokens=N_NEW, eos_token_id=-1)
    next(stream); next(stream)
    assert m.model.lora.shadow_live and m._shadow_depth == 1                # mid-stream: the shadow is in place ...
    changed = [key for key, t in snap[0].items() if not isinstance(key, str) and not torch.equal(m.model.llm.layers[key[0]][key[1]], t)]
    assert changed, "mid-stream the plain weights hold the merge"
    stream.close()
    _assert_untouched(m, snap, "generate_stream closed early")             # ... and gone when the consumer stops
    with pytest.raises(ZeroDivisionError):
        with m.adapters_merged():
            with m.adapters_merged():                                        # re-entrant
                assert m.model.lora.shadow_live and m._shadow_depth == 2
            assert m.model.lora.shadow_live
            1 / 0
    _assert_untouched(m, snap, "an exception inside adapters_merged()")


def _engine_batch(cfg, dev):
    batch = OM.make_batch(cfg, 2, ragged=True)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    gb["masks_list"] = [x.to(dev) for x in batch["masks_list"]]
    return gb


def _engine(m, lr):
    from medplib_amd import engine
    return engine.initialize(model=m, model_parameters=m.trainable_parameters(),
                             config={"optimizer": {"params": {"lr": lr, "betas": (0.9, 0.95)}}, "gradient_clipping": 1.0})[0]


def _step(eng, gb):
    out = eng(**gb)
    loss = float(out["loss"].detach())
    eng.backward(out["loss"])
    eng.step()
    return loss


def test_an_evaluate_between_two_steps_changes_neither(dev):
    """Dense, lora_dropout 0.05 (its mask is keyed on lora.step): step / evaluate() / step against step / step from the same seed."""
    spec = SPECS["dense-all7-r16"]
    runs = []
    for with_eval in (True, False):
        cfg, m = _build(dev, spec, dropout=0.05)
        m.train()
        eng, gb = _engine(m, 1e-3), _engine_batch(cfg, dev)
        l1 = _step(eng, gb)
        if with_eval:
            b, clip, sam = _inputs(cfg, dev)
            snap = _snapshot(m)
            m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=N_NEW, eos_token_id=-1)
            _assert_untouched(m, snap, "evaluate between steps")
            assert m.training
        l2 = _step(eng, gb)
        torch.cuda.synchronize()
        runs.append((l1, l2, [p.detach().clone() for p in m.model.lora.params]))
    (a1, a2, pa), (b1, b2, pb) = runs
    print(f"losses with evaluate() between: {a1!r}, {a2!r}; without: {b1!r}, {b2!r}")
    assert a1 == b1 and a2 == b2 and a1 != a2
    assert len(pa) == len(pb) and all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert any(bool((p != 0).any()) for n, p in zip(m.model.lora.names, pa) if "lora_B" in n)      # (the steps trained the adapters)


def test_a_stale_shadow_is_rebuilt(dev):
    """One adapters_merged() block: evaluate, an optimizer step (ops.PARAM_EPOCH moves), evaluate again = an evaluate() in a fresh block."""
    cfg, m = _build(dev, SPECS["dense-all7-r16"])
    m.train()
    eng, gb = _engine(m, 0.05), _engine_batch(cfg, dev)
    b, clip, sam = _inputs(cfg, dev)
    seen = _capture_hidden(m)

    def ev():
        ids, masks = m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=N_NEW, eos_token_id=-1)
        return ids.clone(), masks[0].float().cpu(), seen["hidden"].float().cpu()

    with m.adapters_merged():
        epoch = ops.PARAM_EPOCH
        first = ev()
        assert m.model.lora.shadow_epoch == epoch
        _step(eng, gb)
        assert ops.PARAM_EPOCH != epoch and m.model.lora.shadow_epoch == epoch and m.model.lora.shadow_live
        second = ev()
        assert m.model.lora.shadow_epoch == ops.PARAM_EPOCH
    fresh = ev()
    assert _equal(second, fresh), "the second evaluate() decoded a stale shadow"
    assert not torch.equal(first[2], second[2]), "the optimizer step must change what is decoded"
    assert not m.model.lora.shadow_live and m._shadow_depth == 0


@pytest.mark.parametrize("name", list(SPECS))
def test_decode_launches_are_the_adapter_less_models(dev, name):
    w = _world(dev, name)
    live, base, (b, clip, _) = w["live"], w["base"], w["inp"]
    for graph in _paths(live):
        traces = []
        for m in (base, live):
            m.decode_with_graph = graph
            m.generate(b["input_ids"], images=clip, max_new_tokens=N_NEW, eos_token_id=-1)          # (first-use caches filled outside the trace)
            with _traced() as calls:
                m.generate(b["input_ids"], images=clip, max_new_tokens=N_NEW, eos_token_id=-1)
            traces.append(list(calls))
        plain, mine = traces
        assert plain and not any("lora_merge" in c for c in plain)
        starts = [p for p in range(len(mine) - len(plain) + 1) if mine[p:p + len(plain)] == plain]
        assert starts, f"{name}, graph={graph}: the adapter-less model's {len(plain)} launches are not a contiguous part of the {len(mine)} with adapters"
        p = starts[0]
        before, after = mine[:p], mine[p + len(plain):]
        assert sum(c.startswith("mp_lora_merge_rows_batched(") for c in before) == 1, before
        assert not any("lora_merge" in c for c in after)
        print(f"{name}, graph={graph}: {len(before)} launches before the prefill, {len(plain)} shared, {len(after)} after the last step")


def test_refusals(dev, tmp_path):
    w = _world(dev, "top1-e2-qv-mlp-r8")
    m, (b, clip, sam) = w["live"], w["inp"]
    snap = _snapshot(m)
    with pytest.raises(RuntimeError, match="merge_and_unload"):
        m.hf_state_dict()
    with m.adapters_merged():
        with pytest.raises(RuntimeError, match="adapters_merged"):
            m.merge_and_unload()
        with pytest.raises(RuntimeError, match="adapters_merged"):
            m.save_pretrained(str(tmp_path / "out"))
        with pytest.raises(RuntimeError, match="adapters_merged"):
            m.save_pretrained(str(tmp_path / "out"), state_dict={})
    assert not (tmp_path / "out").exists()
    _assert_untouched(m, snap, "refused calls")
    m.model.llm.ep = object()                       # a stub: expert parallelism is refused before anything looks at it
    try:
        for call in (lambda: m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=4),
                     lambda: m.generate(b["input_ids"], images=clip, max_new_tokens=4),
                     lambda: list(m.generate_stream(b["input_ids"], clip, max_new_tokens=4)),
                     lambda: m.adapters_merged().__enter__()):
            with pytest.raises(RuntimeError, match="expert parallelism"):
                call()
    finally:
        m.model.llm.ep = None
    _assert_untouched(m, snap, "refused under expert parallelism")
    assert isinstance(np.asarray(m.generate(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1)), np.ndarray)
