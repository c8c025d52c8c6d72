"""The decode entry points, pinned end to end: evaluate / generate / generate_sample / generate_stream / generate_beam on the tiny dense, top-1
and top-2 models, through the captured graph and through the token-by-token loop.  Per case: the ordered list of C-ABI launches of the whole call
(test_gpu_launch_trace._traced: entry point, every scalar argument, whether each pointer is null), last_decode_path, how far llm.gate_pass moved,
and a SHA-256 of what came back (ids; where they exist the mask bytes, last_beam_scores and every yield as (ids, stopped, mask is None)), against
tests/golden/generate_traces.json.  A host-side change of the decode drivers alters none of them.

The fixture is this module's own output at the commit written inside it (`python tests/test_gpu_generate_trace.py --record PATH [--commit HASH]`).
Regenerate it only with a change that is MEANT to alter what a decode call launches or returns, from the parent of that change.  To stay small it
keeps, per case, the SHA-256 of the joined launch list, its length, and the distinct entry points in order of first appearance with their counts
("name*count ..."), so that a mismatch names the entry point whose launches changed; a changed argument shows in the SHA-256 alone.

Every case starts from llm.gate_pass = 0 with no gate draws cached, so a case does not depend on the ones before it."""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                # (run as a script: --record)

from oracle import model as OM  # noqa: E402
from test_gpu_beam_generate import RUNS  # noqa: E402
from test_gpu_launch_trace import _sha, _traced  # noqa: E402
from test_gpu_stream import KINDS, _inputs, _tiny  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_traces.json")
N_NEW = 16                      # one look of the default schedule (every 16 tokens); generate_stream's looks are its yields
_WORLDS = {}


def _world(dev, kind):
    """Per model kind, built once: the model, one prompt, its greedy answer (what the eos of the early-stop case is taken from) and the beam runs' eos."""
    if kind not in _WORLDS:
        cfg, m = _tiny(dev, kind)
        b, clip, sam = _inputs(cfg, dev)
        m.decode_with_graph = False
        free = m.generate(b["input_ids"], images=clip, max_new_tokens=N_NEW, eos_token_id=-1)[0, b["input_ids"].shape[1]:].tolist()
        # the beam runs' eos: the real one (2), or token j of that prompt's greedy answer, so that hypotheses finish and the search is done early
        beam_eos = {}
        for nb in (2, 4):
            for seed, which in RUNS[(kind, nb)]:
                bb, cc, _ = _inputs(cfg, dev, seed=seed)
                beam_eos[(seed, which)] = 2 if which == "real" else int(
                    m.generate(bb["input_ids"], images=cc, max_new_tokens=N_NEW, eos_token_id=-1)[0, bb["input_ids"].shape[1] + which])
        # whatever a model computes once and keeps (the prompt encoder's dense positional tokens, grown tables, workspaces) happens here, not in
        # whichever case runs first
        for graph in (True, False):
            m.decode_with_graph = graph
            m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=4, eos_token_id=-1)
            list(m.generate_stream(b["input_ids"], clip, temperature=0.8, apply_top_p=True, top_k=8, top_p=0.9, max_new_tokens=4, eos_token_id=-1))
            m.generate_beam(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1, num_beams=2)
        _WORLDS[kind] = dict(cfg=cfg, m=m, b=b, clip=clip, sam=sam, free=free, beam_eos=beam_eos)
    return _WORLDS[kind]


def _evaluate(eos_at=None):
    def run(w, dev):
        m, b = w["m"], w["b"]
        eos = -1 if eos_at is None else w["free"][eos_at]
        ids, masks = m.evaluate(w["clip"], w["sam"], b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=N_NEW, eos_token_id=eos)
        n_new = ids.shape[1] - b["input_ids"].shape[1]
        assert n_new == (N_NEW if eos_at is None else eos_at + 1)
        return {"ids": ids.tolist(), "masks": [_sha(x) for x in masks]}, {}
    return run


def _generate_ragged(w, dev):
    b = OM.make_batch(w["cfg"], 2, ragged=True)
    att = b["attention_mask"]
    assert int(att[0].sum()) != int(att[1].sum())
    out = w["m"].generate(b["input_ids"], images=b["images_clip"].to(dev).to(torch.bfloat16), attention_mask=att, max_new_tokens=N_NEW, eos_token_id=-1)
    return {"ids": out.tolist()}, {}


def _sample(**kw):
    def run(w, dev):
        out = w["m"].generate_sample(w["b"]["input_ids"], images=w["clip"], max_new_tokens=N_NEW, eos_token_id=-1, temperature=0.8, sample_seed=11, **kw)
        return {"ids": out.tolist()}, {}
    return run


def _stream(abandon_after=None, **kw):
    def run(w, dev):
        m = w["m"]
        if abandon_after is not None:
            m.train(True)                       # the consumer walks away: the mode and the adapters must come back all the same
        gen = m.generate_stream(w["b"]["input_ids"], w["clip"], max_new_tokens=N_NEW, eos_token_id=-1, **kw)
        ys = []
        for y in gen:
            ys.append([list(y[0]), bool(y[1]), y[2] is None])
            if len(ys) == abandon_after:
                break
        gen.close()
        state = {}
        if abandon_after is not None:
            state = {"training_after": m.training, "llm_training_after": m.model.llm.training, "shadow_depth": m._shadow_depth,
                     "adapters": getattr(m.model, "lora", None) is not None}
            assert state["training_after"] and state["shadow_depth"] == 0
            m.train(False)
        return {"yields": ys}, state
    return run


def _uniforms(i):
    return ((i * 37 + 11) % 101) / 101.0


def _beam(nb):
    def run(w, dev):
        m, cfg = w["m"], w["cfg"]
        out = {}
        for seed, which in RUNS[(w["kind"], max(nb, 2))]:
            b, clip, _ = _inputs(cfg, dev, seed=seed)
            eos = w["beam_eos"][(seed, which)]
            ids = m.generate_beam(b["input_ids"], images=clip, max_new_tokens=N_NEW, eos_token_id=eos, num_beams=nb)
            out[f"{seed}-{which}"] = {"ids": ids.tolist(), "scores": [repr(float(s)) for s in m.last_beam_scores]}
        return out, {}
    return run


CASES = {
    "evaluate": _evaluate(),
    "evaluate-eos-at-6": _evaluate(eos_at=5),                                  # the stop falls between two looks: the replays after it are discarded
    "generate-ragged-B2": _generate_ragged,
    "sample-unfiltered": _sample(top_k=0, top_p=1.0),
    "sample-k50-p0.9": _sample(top_k=50, top_p=0.9),
    "stream-greedy-interval-4": _stream(temperature=0.0, stream_interval=4),
    "stream-T0.8": _stream(temperature=0.8, sample_seed=7),
    "stream-T0.8-k8-p0.9": _stream(temperature=0.8, sample_seed=7, apply_top_p=True, top_k=8, top_p=0.9),
    "stream-injected-uniforms": _stream(temperature=0.8, uniforms=_uniforms),  # a host-side provider forces the loop
    "stream-abandoned-after-2": _stream(abandon_after=2, temperature=0.8, sample_seed=7, stream_interval=4),
    "beam-1": _beam(1),
    "beam-2": _beam(2),
    "beam-4": _beam(4),
}
PARAMS = [(name, kind, graph) for name in CASES for kind in KINDS for graph in (True, False)]


def _key(name, kind, graph):
    return f"{name}-{kind}-{'graph' if graph else 'loop'}"


def _run(name, kind, graph, dev):
    w = dict(_world(dev, kind), kind=kind)
    m, llm = w["m"], w["m"].model.llm
    assert m._graph_decode_ok()                 # the three tiny models all take the captured graph
    m.decode_with_graph = graph
    m.train(False)
    llm.gate_pass, llm._draws_key, m.last_decode_path = 0, None, None
    with _traced() as calls:
        out, state = CASES[name](w, dev)
    torch.cuda.synchronize()
    counts = {}
    for c in calls:
        counts[c.split("(")[0]] = counts.get(c.split("(")[0], 0) + 1
    state = dict(state, path=m.last_decode_path, gate_pass=llm.gate_pass)
    return {"calls_sha256": hashlib.sha256("\n".join(calls).encode()).hexdigest(), "n_calls": len(calls),
            "entry_points": " ".join(f"{k}*{v}" for k, v in counts.items()),
            "sha256": hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest(), "state": state}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_commit_and_every_case(recorded):
    assert len(recorded["commit"]) == 40 and set(recorded["cases"]) == {_key(*p) for p in PARAMS}


@pytest.mark.parametrize("name,kind,graph", PARAMS, ids=[_key(*p) for p in PARAMS])
def test_generate_trace(dev, recorded, name, kind, graph):
    got, want = _run(name, kind, graph, dev), recorded["cases"][_key(name, kind, graph)]
    host_pick = name == "stream-injected-uniforms"
    assert got["state"]["path"] == ("graph" if graph and not host_pick else "loop")
    assert got["entry_points"] == want["entry_points"], f"launches per entry point differ: {got['entry_points']} / recorded {want['entry_points']}"
    assert got["n_calls"] == want["n_calls"]
    assert got["calls_sha256"] == want["calls_sha256"], "the same entry points, but an argument or the order of the launches changed"
    assert got["state"] == want["state"]
    assert got["sha256"] == want["sha256"], "what the call returned changed"


if __name__ == "__main__":
    import argparse
    import subprocess
    import time
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="PATH")
    ap.add_argument("--commit", default=None, help="hash of the commit being recorded (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    t0 = time.time()
    cases = {_key(*p): _run(*p, torch.device("cuda:0")) for p in PARAMS}
    with open(a.record, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(cases)} cases, {sum(c['n_calls'] for c in cases.values())} launches at {commit} in {time.time() - t0:.1f} s -> {a.record}")
