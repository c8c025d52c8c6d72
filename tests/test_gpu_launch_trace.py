"""The decoder stack's host side, pinned: for every branch of LlamaStack.forward / decode_step and of llama_lora.forward_train + backward, the
ordered list of C-ABI launches (entry point, every non-pointer argument, whether each pointer argument is null) and a SHA-256 of the bytes that
come back, against tests/golden/launch_traces.json.  A host-side clean-up of the stack changes neither; a changed branch order, condition,
scalar argument or a pointer that became None shows up here by name.

The fixture is this module's own output at the commit written inside it (`python tests/test_gpu_launch_trace.py --record PATH [--commit HASH]`);
the stacks seed their weights from a device generator and every input below from a CPU generator, so the bytes reproduce.  Regenerate it only
with a change that is MEANT to alter a launch sequence, from the parent of that change.  The two once-per-process workspace registrations are left
out of the lists (whether they happen inside a case depends on what ran before it).

The training cases cover the dense adapters (MLP targets; all seven targets at r = 16 and at r = 8 with dropout; frozen input rows; trainable norms;
a gradient sink with and without the weight-gradient stream; d = 4096 for the up-projection deferred into the norm backward) and the MoE layers
(top-1 with and without dropout, top-2, and the expert-parallel branch on a one-rank group, whose exchanges are identities)."""
import contextlib
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")
_ONCE_PER_PROCESS = ("mp_gemm_set_workspace", "mp_gemm_set_stream_workspace")


@contextlib.contextmanager
def _traced():
    """Record every _Lib.call / _Lib.raw call made inside the block as "name(arg,...)": a scalar argument by value, a pointer (or stream) as * / -."""
    from medplib_amd import _lib
    L = _lib.lib()
    cls, calls = type(L), []
    orig_call, orig_raw = cls.call, cls.raw

    def note(name, args):
        if name in _ONCE_PER_PROCESS:
            return
        out = []
        assert len(args) == len(L.protos[name][1]), name
        for (ctype, _), a in zip(L.protos[name][1], args):
            a = getattr(a, "value", a)                     # (ctypes.c_void_p(...) wrappers)
            if ctype.endswith("*") or ctype == "hipStream_t":
                out.append("*" if a else "-")
            elif ctype == "float":
                out.append(repr(float(a)))
            else:
                out.append(str(int(a)))
        calls.append(f"{name}({','.join(out)})")

    def call(self, name, *args):
        note(name, args)
        return orig_call(self, name, *args)

    def raw(self, name):
        fn = orig_raw(self, name)

        def traced_fn(*args):
            note(name, args)
            return fn(*args)
        return traced_fn

    cls.call, cls.raw = call, raw
    try:
        yield calls
    finally:
        cls.call, cls.raw = orig_call, orig_raw


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _cfg(kind, **kw):
    from medplib_amd.model.config import MedPLIBConfig
    base = {"dense": dict(moe_enable=False), "top1": dict(moe_enable=True), "top2": dict(moe_enable=True, top_k_experts=2)}[kind]
    return MedPLIBConfig.tiny(**dict(base, **kw))


def _stack(dev, cfg):
    from medplib_amd.model.llama import LlamaStack
    return LlamaStack(cfg, dev, seed=7)


def _embeds(dev, B, S, d, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, d, generator=g) * 0.5).to(torch.bfloat16).to(dev)


B_ROWS, S_ROWS = 2, 13          # 26 rows: above the 8-row GEMV threshold, odd sequence length, capacity (20) below the row count


def _forward_case(kind="top1", cfg_kw=None, fuse=True, needed=None, collect=False):
    def run(dev):
        llm = _stack(dev, _cfg(kind, **(cfg_kw or {})))
        llm.fuse_moe_gather_scatter = fuse
        x = _embeds(dev, B_ROWS, S_ROWS, llm.cfg.hidden_size)
        if needed is not None:
            mask = torch.zeros(B_ROWS * S_ROWS, dtype=torch.uint8)
            mask[list(needed)] = 1
            llm.needed_rows = (mask.nonzero().flatten().to(dev), mask.to(dev))
        with _traced() as calls:
            out, aux, routing = llm.forward(x, collect_routing=collect)
        llm.needed_rows = None
        sha = {"hidden": _sha(out)}
        if aux:
            sha["aux"] = _sha(torch.cat([a.reshape(1) for a in aux]))
        state = {"folded_layers": llm.folded_layers, "pruned_rows": llm.pruned_rows, "gate_pass": llm.gate_pass, "aux": len(aux)}
        if collect:
            sha["last_gate_inputs"] = _sha(torch.cat(llm.last_gate_inputs))
            sha["routing"] = _sha(torch.cat([t.reshape(-1).to(torch.int64) for r in routing for t in r]))
        return calls, sha, state
    return run


def _cached_case(kind, B):
    def run(dev):
        llm = _stack(dev, _cfg(kind))
        llm.training = False
        d = llm.cfg.hidden_size
        cache = llm.new_kv_cache(B, 32)
        with _traced() as calls:
            pre, _, _ = llm.forward(_embeds(dev, B, S_ROWS, d), kv_cache=cache)
            tok, _, _ = llm.forward(_embeds(dev, B, 1, d, seed=2), kv_cache=cache)
        return calls, {"prefill": _sha(pre), "token": _sha(tok), "k_last": _sha(cache["k"][-1][:, :S_ROWS + 1])}, {"len": cache["len"], "gate_pass": llm.gate_pass}
    return run


def _decode_case(kind, B, fuse_routing, d):
    def run(dev):
        # d = 512 is a size ops.gemv_rmsnorm_ok accepts (the norm-folded GEMVs), 256 one it refuses; a capacity factor of 0.5 puts two top-1 rows over
        # capacity (cap 1 < B = 2: the draws are generated), one row not (cap 1 >= B = 1: no draws)
        llm = _stack(dev, _cfg(kind, hidden_size=d, num_attention_heads=d // 128, moe_gate_sampling=True, eval_capacity_factor=0.5))
        llm.training = False
        llm.fuse_decode_routing = fuse_routing
        cache = llm.new_kv_cache(B, 32)
        llm.forward(_embeds(dev, B, 5, d), kv_cache=cache)                      # (prefill: traced by the cached-forward cases)
        counters = torch.tensor([5, 6], dtype=torch.int32, device=dev)
        pass_dev = torch.tensor([llm.gate_pass + 1], dtype=torch.int32, device=dev)
        with _traced() as calls:
            h = llm.decode_step(_embeds(dev, B, 1, d, seed=2), cache, counters, pass_dev=pass_dev)
        return calls, {"hidden": _sha(h), "k_last": _sha(cache["k"][-1][:, :6]), "err": _sha(cache["err"])}, {"gate_pass": llm.gate_pass}
    return run


def _folded_case(dev):
    """The shape of tests/test_gpu_fold_norm.py: the fold needs head_dim 128 and at least 1024 rows of a 320-row-kernel shape."""
    from medplib_amd.model.config import MedPLIBConfig
    from medplib_amd.model.llama import LlamaStack
    llm = LlamaStack(MedPLIBConfig.medplib_7b(fold_input_norm=True, num_hidden_layers=2, vocab_size=1024, moe_enable=True), dev, seed=5)
    x = _embeds(dev, 3, 512, 4096, seed=9)
    with _traced() as calls:
        out, aux, _ = llm.forward(x)
    return calls, {"hidden": _sha(out), "aux": _sha(torch.cat([a.reshape(1) for a in aux]))}, {"folded_layers": llm.folded_layers, "pruned_rows": llm.pruned_rows}


def _train_case(needed=None, kind="dense", cfg=None, targets=("gate_proj", "up_proj", "down_proj"), r=8, dropout=0.0, sft_modules=(), need_d_embeds=True,
                sink=False, wgrad_stream=False, d_aux=False, ep=False):
    """forward_train + backward.  cfg: a callable that builds the config (default: the tiny one of `kind`); sink: the parameters' .grad preallocated
    and a gradient sink attached (the .grad tensors are hashed, and the sink's calls go into the state); wgrad_stream: llama_lora._WGRAD_STREAM for the
    pass; d_aux: the MoE layers' l_aux gradient given; ep: a one-rank expert-parallel group (the exchanges are identities)."""
    def run(dev):
        from medplib_amd.model import llama_lora
        c = cfg() if cfg is not None else _cfg(kind)
        llm = _stack(dev, c)
        comm = None
        if ep:
            from medplib_amd.comm import RcclComm
            from medplib_amd.expert_parallel import ExpertParallel
            comm = RcclComm(rank=0, world=1)
        try:
            if ep:
                llm.enable_expert_parallel(ExpertParallel(None, 1, c.num_experts, capi_comm=comm))
            lora = llama_lora.enable_lora(llm, c, r=r, alpha=16, dropout=dropout, targets=targets, sft_modules=sft_modules)
            llm.training = True
            g = torch.Generator().manual_seed(31)
            for n, p in zip(lora.names, lora.params):
                p.data.copy_((torch.randn(p.shape, generator=g) * (0.05 if "lora_A" in n else 0.03)).to(torch.bfloat16).float().to(dev))
            x = _embeds(dev, B_ROWS, S_ROWS, c.hidden_size)
            dy = _embeds(dev, B_ROWS, S_ROWS, c.hidden_size, seed=3)
            if needed is not None:
                mask = torch.zeros(B_ROWS * S_ROWS, dtype=torch.uint8)
                mask[list(needed)] = 1
                llm.needed_rows = (mask.nonzero().flatten().to(dev), mask.to(dev))
                dy = dy * mask.view(B_ROWS, S_ROWS, 1).to(dev).to(dy.dtype)       # nothing reads the other rows: their gradient is zero
            handed = []
            if sink:
                for p in lora.params:
                    p.grad = torch.zeros(p.shape, dtype=torch.float32, device=dev)
                lora.grad_sink = lambda i, ng: handed.append((i, ng))
            aux_grad = torch.tensor([0.01], dtype=torch.float32, device=dev) if d_aux else None
            was = llama_lora._WGRAD_STREAM
            llama_lora._WGRAD_STREAM = wgrad_stream
            try:
                with torch.no_grad(), _traced() as calls:
                    out, aux_sum, saved = llama_lora.forward_train(llm, x, None)
                    grads = llama_lora.backward(llm, saved, dy, aux_grad, need_d_embeds=need_d_embeds)
            finally:
                llama_lora._WGRAD_STREAM = was
            llm.needed_rows = None
            sha = {"hidden": _sha(out)}
            sha.update({"grad:" + n: _sha(grads[n]) for n in sorted(grads) if grads[n] is not None})
            state = {"pruned_rows": llm.pruned_rows, "gate_pass": llm.gate_pass, "grads": len(grads)}
            if d_aux:
                sha["aux_sum"] = _sha(aux_sum)
            if sink:
                sha.update({"param.grad:" + n: _sha(p.grad) for n, p in zip(lora.names, lora.params)})
                sha.update({f"sink:{i}:{n}": _sha(t) for i, ng in handed for n, t in ng.items()})
                state["sink"] = [[i, sorted(ng)] for i, ng in handed]
            if not need_d_embeds:
                state["d_embeds_is_none"] = grads["__d_embeds__"] is None
            return calls, sha, state
        finally:
            if comm is not None:
                comm.close()
    return run


def _d4096_one_layer():
    from medplib_amd.model.config import MedPLIBConfig
    return MedPLIBConfig.medplib_7b(num_hidden_layers=1, vocab_size=1024, moe_enable=False)


FEW_ROWS = (3, 11, 25)
ALL_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
MLP_AND_QV = ("gate_proj", "up_proj", "down_proj", "q_proj", "v_proj")

CASES = {
    "forward-dense": _forward_case("dense"),
    "forward-top1-gather-scatter": _forward_case("top1"),
    "forward-top1-gather-scatter-needed-rows": _forward_case("top1", needed=FEW_ROWS),
    "forward-top1-unfused": _forward_case("top1", fuse=False),
    "forward-top2": _forward_case("top2"),
    "forward-residual": _forward_case("top1", cfg_kw=dict(use_residual=True)),
    "forward-top1-gate-sampling": _forward_case("top1", cfg_kw=dict(moe_gate_sampling=True)),
    "forward-top1-collect-routing": _forward_case("top1", collect=True),
    "forward-top1-norm-gate-d2048": _forward_case("top1", cfg_kw=dict(hidden_size=2048, num_attention_heads=16)),     # (an ops.RMSNORM_GATE_DIMS size: norm + gate in one launch)
    "folded-norms": _folded_case,
    "train-dense-adapters": _train_case(None),
    "train-dense-adapters-needed-rows": _train_case(FEW_ROWS),
    "train-dense-all-targets-r16": _train_case(targets=ALL_TARGETS, r=16),                     # qkv R = 48 -> 64 (the R > 32 fallbacks), gu R = 32, o / down R = 16
    "train-dense-all-targets-r8-dropout": _train_case(targets=ALL_TARGETS, dropout=0.1),       # keep-bits at K = 256, refused at K = 320; qkv R = 24 -> 32
    "train-dense-frozen-inputs": _train_case(need_d_embeds=False),                             # layer 0 stops at the gate|up gradient
    "train-dense-norms-trainable": _train_case(FEW_ROWS, sft_modules=("input_layernorm", "post_attention_layernorm")),     # ln2 trains: no pruning
    "train-dense-grad-sink": _train_case(sink=True),                                           # chunk partials unpacked straight into .grad
    "train-dense-grad-sink-wgrad-stream": _train_case(sink=True, wgrad_stream=True),           # the same launches in host order, on two queues
    "train-top1-adapters": _train_case(kind="top1", d_aux=True),                               # fused capacity slabs, gate backward, d wg
    "train-top1-adapters-dropout": _train_case(kind="top1", d_aux=True, dropout=0.1),          # per-expert seeds
    "train-top2-adapters": _train_case(kind="top2", d_aux=True),
    "train-top1-expert-parallel-one-rank": _train_case(kind="top1", d_aux=True, dropout=0.1, ep=True, targets=MLP_AND_QV),
    "train-dense-d4096-one-layer": _train_case(cfg=_d4096_one_layer),                          # d == 4096: the deferred up-projection in the norm backward
}
for _kind in ("dense", "top1", "top2"):
    for _B in (1, 2):
        CASES[f"cached-forward-{_kind}-B{_B}"] = _cached_case(_kind, _B)
        for _d in (512, 256):
            for _fuse in (True, False):
                CASES[f"decode-step-{_kind}-B{_B}-d{_d}-routing-{'fused' if _fuse else 'separate'}"] = _decode_case(_kind, _B, _fuse, _d)


def _run(name, dev):
    calls, sha, state = CASES[name](dev)
    return {"calls": calls, "sha256": sha, "state": state}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_commit_and_every_case(recorded):
    assert len(recorded["commit"]) == 40 and set(recorded["cases"]) == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_trace(dev, recorded, name):
    got, want = _run(name, dev), recorded["cases"][name]
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}: launch {k} differs"
    assert len(got["calls"]) == len(want["calls"]), f"{name}: {len(got['calls'])} launches, recorded {len(want['calls'])}"
    assert got["state"] == want["state"]
    assert got["sha256"] == want["sha256"]
    if name == "forward-top1-gather-scatter-needed-rows" or name == "train-dense-adapters-needed-rows":
        assert got["state"]["pruned_rows"] == len(FEW_ROWS)
    if name == "folded-norms":
        assert got["state"]["folded_layers"] == 2


if __name__ == "__main__":
    import argparse
    import subprocess
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="PATH")
    ap.add_argument("--commit", default=None, help="hash of the commit being recorded (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=root, text=True).strip()
    t0 = time.time()
    cases = {name: _run(name, torch.device("cuda:0")) for name in CASES}
    with open(a.record, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(cases)} cases, {sum(len(c['calls']) for c in cases.values())} launches at {commit} in {time.time() - t0:.1f} s -> {a.record}")
