"""Token generation of `MedPLIBForCausalLM`: evaluate / generate / generate_sample / generate_beam / generate_stream over ONE decode driver.

A call is: the decode prologue (`_decoding`), one prefill (`_prefill`), then `_drive` with a selection policy.  `_drive` takes the first step's
logits from the prefill and hands the rest to one of two drivers:

* `_captured_steps`: one step captured into a HIP graph and replayed once per token; the host reads the step records (and the cache's error
  word, in the same copy) only at the looks;
* `_loop_steps`: the token-by-token loop over `LlamaStack.forward`, a host read per token.

A policy says what a step selects and what the host keeps of it: `_single_row_policy` (one sequence, the next token chosen by a pick — the greedy
argmax or a `_SamplePick`), `_beam_policy` (the num_beams beams of one prompt as the rows of one step) and `_batch_policy` (several prompts of
different lengths as the rows of one step, each with its own position and key count, optionally its own limit and stop ids; picked greedily
(generate_batch) or by a `_RowsPick`, every row at its own request's sampling parameters: generate_sample_batch, generate_stream_batch).
Each is a namespace of closures:

    first(logits)        the selection of step 0, from the prefill's logits
    step(forward, at)    one decode step: embed the selected ids, forward(emb) -> hidden, logits, selection.  `at` is the device counters of a
                         captured step ([position, keys after it] + [token number] with needs_step) or the token number in the loop
    file(i)              called after step i was computed (after every replay, outside the graph): keep its record
    records(upto), look(bytes, upto) -> (kept steps, done, what to yield)      the captured driver's read at a look
    loop_look(i) -> (finished, what to yield)                                  the loop's read after step i
    reorder              the loop's hook before a step (beams: HF's whole-cache _reorder_cache), or None
    counters, forward    None, or (the batch policy) counters() -> the initial device counters of the call and forward(emb, counters, pass_dev)
                         -> hidden, the decode step both drivers then run: the loop too, advancing the counters after every step
    needs_step, debug, n_dbg, err_also"""
import contextlib
import dataclasses
import types

import numpy as np
import torch

from .. import ops


def _h2d(arr, device):
    """Host index array -> device tensor without stalling the host: a pageable-memory copy is synchronous for the caller AND
    ordered behind everything already queued on the stream, so one such copy after the LLM launches makes the host wait for the
    whole stack (measured: 66 of 97 ms per step spent blocked in .to()).  Pinned staging + non_blocking lets the host run ahead and
    queue the SAM encoder / mask tail while the LLM is still executing."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    return t.pin_memory().to(device, non_blocking=True)


def _np_ids(t):
    if isinstance(t, np.ndarray):
        return t
    return t.detach().cpu().numpy()


# HF generate kwargs the entry points accept when they mean what the entry point does (the reference driver's set, vqa_infer.py:430-442)
_GENERATE_KWARGS = frozenset({"do_sample", "temperature", "top_p", "num_beams", "use_cache", "mask_images", "image_token_types",
                              "image_token_lengths", "region_masks", "valid_region_masks_bool", "output_hidden_states",
                              "return_dict_in_generate", "pad_token_id"})
# what an entry point refuses loudly instead of decoding something else than was asked for
_REFUSED = {
    "generate": {"sampling": "sampling (do_sample / temperature > 0) is not built here: call generate_sample() (temperature, top-k, top-p); "
                             "the shipped eval scripts decode greedily",
                 "beams": "beam search (num_beams > 1) is not built here: call generate_beam(); the shipped eval scripts use num_beams=1"},
    "generate_sample": {"beams": "beam search (num_beams > 1) is not built; the shipped eval scripts use num_beams=1"},
    "generate_sample_batch": {"beams": "beam search per batch row (num_beams > 1) is not built: call generate_beam()"},
    "generate_beam": {"sampling": "beam sampling (do_sample / temperature > 0 with num_beams > 1) is not built"},
    "generate_batch": {"sampling": "sampling per batch row (do_sample / temperature > 0) is not built: the rows of a batch are decoded greedily; "
                                   "call generate_sample()",
                       "beams": "beam search per batch row (num_beams > 1) is not built: call generate_beam()"},
}


def _check_kwargs(who, kwargs, extra_allowed=()):
    """The HF generate kwargs of entry point `who`: accepted when they mean what it does, NotImplementedError for sampling / beams it does not
    do (_REFUSED), TypeError for anything outside _GENERATE_KWARGS + extra_allowed."""
    asked = {"sampling": kwargs.get("do_sample") or (kwargs.get("temperature") or 0) > 0 and kwargs.get("do_sample") is not False,
             "beams": (kwargs.get("num_beams") or 1) != 1}
    for what, text in _REFUSED[who].items():
        if asked[what]:
            raise NotImplementedError(f"{who}(): {text}")
    unknown = set(kwargs) - _GENERATE_KWARGS - set(extra_allowed)
    if unknown:
        raise TypeError(f"{who}(): unsupported arguments {sorted(unknown)}")


@dataclasses.dataclass(frozen=True)
class PromptExtras:
    """What a prompt carries besides its ids and CLIP images: the ICL mask images and token layout, and the region prompts of the sample."""
    mask_images: object = None
    image_token_types: object = None
    image_token_lengths: object = None
    region_masks: object = ()
    valid_region_masks_bool: object = ()


NO_EXTRAS = PromptExtras()


@dataclasses.dataclass(frozen=True)
class StreamRequest:
    """One request of generate_stream_batch: generate_stream()'s arguments that belong to the request.  input_ids [1, L] and images_clip as
    there; images (the SAM input) with resize_list and original_size_list for the mask of a stopping yield; temperature < 1e-4 is greedy;
    top_p and top_k count only with apply_top_p; the request stops at eos, at stop_token_id, or when stop_check(ids) is true at a yield."""
    input_ids: object
    images_clip: object
    images: object = None
    resize_list: object = None
    original_size_list: object = None
    region_masks: object = ()
    valid_region_masks_bool: object = ()
    temperature: float = 1.0
    top_p: float = 1.0
    top_k: int = 0
    apply_top_p: bool = False
    max_new_tokens: int = 256
    stop_token_id: object = None
    sample_seed: int = 0
    stop_check: object = None


def _argmax_pick(logits, step):
    """The greedy next-token pick (HF do_sample=False).  `step` (the number of the generated token) is not used."""
    return ops.argmax_rows(logits)


class _SamplePick:
    """The sampling next-token pick of generate_stream: token `step` of a request is ops.sample_rows at the uniform the keyed generator
    draws under (seed, step).  `step` is an int (the first token, the token-by-token loop) or an int32 [1] device counter (the captured
    decode step: every replay draws what the loop draws for that token).  An injected `uniforms(step) -> float` replaces the generator; it
    runs on the host, so it cannot be captured.  last_u: the [1] tensor of the latest draw (inside a captured step: the graph's own buffer).
    top_k / top_p truncate the distribution first (ops.sample_rows_filtered: HF's top-k, then top-p); with both off (0 and 1.0) the pick is
    ops.sample_rows as before.  Temperature, top_k and top_p are launch constants of a captured step."""
    needs_step = True                        # the captured step keeps the number of the generated token on the device

    def __init__(self, temperature, seed, device, uniforms=None, top_k=0, top_p=1.0):
        self.temperature, self.seed, self.device, self.uniforms, self.last_u = float(temperature), int(seed), device, uniforms, None
        self.top_k, self.top_p = int(top_k), float(top_p)
        if self.top_k < 0 or not 0.0 <= self.top_p <= 1.0:
            raise ValueError(f"sampling: top_k={top_k} must not be negative and top_p={top_p} must lie in [0, 1]")

    def __call__(self, logits, step):
        if self.uniforms is not None:
            u = torch.tensor([float(self.uniforms(int(step)))], dtype=torch.float32, device=self.device)
        elif torch.is_tensor(step):
            u = ops.sample_uniform_dev(self.seed, step, self.device)
        else:
            u = ops.sample_uniform(self.seed, int(step), self.device)
        self.last_u = u
        if self.top_k == 0 and self.top_p >= 1.0:
            return ops.sample_rows(logits, u, self.temperature)
        return ops.sample_rows_filtered(logits, u, self.temperature, self.top_k, self.top_p)


class _RowsPick:
    """The pick of a batch group whose rows each bring their own request: row b is greedy (temperature None or 0: inv_temperature 0) or
    drawn at its own temperature, top_k and top_p (0 and 1.0: the plain pick) under its own seed.  One draw launch and one pick launch serve
    the group (ops.sample_uniform_rows, ops.pick_rows): token `step` of row b is the single-row op of _SamplePick — or ops.argmax_rows — on
    that row's logits at the keyed draw for (seeds[b], step), bit for bit.  The parameters live in device arrays the launches read, so a
    captured step holds no request constant.  `step`: an int or the captured step's int32 [1] device counter.  last_u: the [B] draws of the
    latest step.  err: the int32 [1] word a row with refused parameters sets (POS_ERR_PICK); _batch_policy hands it the cache's."""
    needs_step = True

    def __init__(self, temperatures, top_ks, top_ps, seeds, device, err=None):
        inv_t = []
        for t, k, p in zip(temperatures, top_ks, top_ps):
            t = 0.0 if t is None else float(t)
            if not (0.0 <= t < float("inf")) or int(k) < 0 or not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"sampling: temperature={t} must be finite and not negative, top_k={k} not negative and top_p={p} in [0, 1]")
            inv_t.append(1.0 / t if t > 0 else 0.0)
        self.inv_temperature = torch.tensor(inv_t, dtype=torch.float32).to(device)
        self.top_k = torch.tensor([int(k) for k in top_ks], dtype=torch.int32).to(device)
        self.top_p = torch.tensor([float(p) for p in top_ps], dtype=torch.float32).to(device)
        self.seeds = torch.tensor([int(s) for s in seeds], dtype=torch.int64).to(device)
        self.device, self.err, self.last_u = device, err, None

    def __call__(self, logits, step):
        if self.err is None:
            self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        u = ops.sample_uniform_rows(self.seeds, step)
        self.last_u = u
        return ops.pick_rows(logits, u, self.inv_temperature, self.top_k, self.top_p, self.err)


# ---------------------------------------------------------------------- the two drivers
def _raise_on_error_word(llm, cache, err, steps=None, S=None, also=""):
    """The cache's error word (MP_POS_ERR_*) after decode steps: non-zero when a bounded kernel met a position without a table or cache row,
    or (POS_ERR_PICK) when the per-row pick met a row whose parameters no pick accepts."""
    if err:
        if err & ops.POS_ERR_PICK:
            also += ", or the per-row pick refused a row's parameters (inv_temperature negative or not finite, top_k < 0, top_p outside [0, 1])"
        if steps is None:
            where = "a decode step"
        elif isinstance(S, (list, tuple)):       # a batch group: every row has its own prompt length
            where = f"decode steps {steps[0]}..{steps[1]} (positions " + ", ".join(f"{n + steps[0] - 1}..{n + steps[1] - 1}" for n in S) + " of the rows)"
        else:
            where = f"decode steps {steps[0]}..{steps[1]} (positions {S + steps[0] - 1}..{S + steps[1] - 1})"
        raise RuntimeError(f"decode: {where} ran past the RoPE table ({llm.cos.shape[0]} rows) or the KV cache ({cache['k'][0].shape[1]} rows)"
                           f"{also}: error word {err}")


def _default_looks(max_new_tokens, check_every=16):
    """The step counts at which the host looks at a captured decode: every `check_every` steps and at the end."""
    return list(range(1 + check_every, max_new_tokens, check_every)) + [max_new_tokens]


def _captured_steps(llm, cache, S, policy, looks):
    """Decode with ONE captured HIP graph per call: policy.step — embed(selected ids) -> 32 decode layers (GEMV projections, RoPE + KV append
    and attention at the device-side cache length) -> final norm -> lm_head -> selection, all on the device — is captured once and replayed
    once per token (~450 kernel launches otherwise); the host looks at what the steps recorded only at `looks`, the step counts at which it
    does, increasing and ending at max_new_tokens.  Steps after the one at which the policy is done are discarded, so the result equals the
    token-by-token loop.  A generator: at every look it yields what policy.look returns."""
    dev = llm.device
    # [position of the fed token, keys after appending it] and, for a pick that draws, the number of the token being generated: one
    # advance per replay bumps them all
    # (a policy with rows of different lengths supplies its own: a position and a key count per row)
    counters = policy.counters() if policy.counters is not None else \
        torch.tensor([S, S + 1] + ([1] if policy.needs_step else []), dtype=torch.int32, device=dev)
    # the gate's random draws (moe_gate_sampling) are keyed on the forward-pass number: the token-by-token loop gives the decode step
    # of token i pass pass0 + i, so the graph reads it from a device counter it advances itself
    pass0 = llm.gate_pass
    pass_dev = torch.tensor([pass0 + 1], dtype=torch.int32, device=dev)

    def step():
        if policy.forward is not None:
            policy.step(lambda emb: policy.forward(emb, counters, pass_dev), counters)
        else:
            policy.step(lambda emb: llm.decode_step(emb, cache, counters, pass_dev=pass_dev), counters)
        ops.advance_ints(counters, 1)
        ops.advance_ints(pass_dev, 1)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    at = kept = 1
    try:
        for upto in looks:
            for i in range(at, upto):
                graph.replay()                                   # feeds the selection of step i-1, computes step i
                policy.file(i)
            # the only host synchronisation of the loop: the steps' records and the cache's error word (MP_POS_ERR_*) in one copy
            got = torch.cat([policy.records(upto).reshape(-1).view(torch.uint8), cache["err"].view(torch.uint8)]).cpu().numpy()
            _raise_on_error_word(llm, cache, int(got[-4:].view(np.int32)[0]), (at, upto - 1), S, policy.err_also)
            at = upto
            kept, done, out = policy.look(got[:-4], upto)
            yield out
            if done:
                break
    finally:                                     # (also when the consumer stops reading early)
        llm.gate_pass = pass0 + max(kept, 1) - 1   # the passes the loop would have made (replays past the last kept step are discarded)
        llm._draws_key = None                    # (the captured draw buffer belongs to the graph)
        if policy.debug is not None:
            del policy.debug[policy.n_dbg + kept:]


def _loop_steps(llm, cache, policy, max_new_tokens):
    """Decode token by token: after every step the host reads it (policy.loop_look) and yields; until the policy has finished, the next step
    runs through LlamaStack.forward against the KV cache — or through the policy's own forward (the batch policy: the decode step of the
    captured driver, uncaptured, at device counters this loop advances)."""
    counters = policy.counters() if policy.forward is not None else None
    for i in range(max_new_tokens):
        finished, out = policy.loop_look(i)
        yield out
        if finished:
            return
        if policy.reorder is not None:
            policy.reorder()
        if policy.forward is not None:
            policy.step(lambda emb: policy.forward(emb, counters, None), i + 1)
            ops.advance_ints(counters, 1)
        else:
            policy.step(lambda emb: llm.forward(emb, None, kv_cache=cache)[0], i + 1)
        policy.file(i + 1)


# ---------------------------------------------------------------------- the three selection policies
def _single_row_policy(llm, hidden, cache, max_new_tokens, stop_ids, pick, debug, captured):
    """One sequence, the next token chosen by `pick`.  Yields (generated ids so far, stopped, [hidden states of the prompt, of each fed
    token]); stops at one of `stop_ids` or at max_new_tokens.  debug: a list that receives (fp32 logits row on the host, u or None, token)
    per kept token."""
    d, dev = llm.cfg.hidden_size, llm.device
    needs_step = getattr(pick, "needs_step", False)
    st = types.SimpleNamespace(tok=None, logits=None)        # the selected token (int64 [1] on the device) and the logits it came from
    generated, hiddens = [], [hidden]                         # the loop's record
    if captured:                                              # the graph's: its output buffer, and what every replay leaves is copied out of it
        toks = torch.empty(max_new_tokens, dtype=torch.int64, device=dev)
        hid_all = torch.empty((max_new_tokens, d), dtype=torch.bfloat16, device=dev)
        h_static = torch.empty((1, 1, d), dtype=torch.bfloat16, device=dev)

    def select(logits, step_no):
        st.logits = logits
        tok = pick(logits, step_no)
        if captured and st.tok is not None:
            st.tok.copy_(tok)                                 # the captured step reads and writes one buffer
        else:
            st.tok = tok

    def step(forward, at):
        emb = ops.splice_rows(llm.embed_tokens, None, st.tok, d)
        h = forward(emb.view(1, 1, d))
        if captured:
            h_static.copy_(h)
            select(llm.next_token_logits(h[0, -1:]), at[2:3] if needs_step else None)
        else:
            hiddens.append(h)
            select(llm.next_token_logits(h[0, -1:]), at)

    def file(i):
        if captured:
            if i:
                hid_all[i - 1:i].copy_(h_static.view(1, d))
            toks[i:i + 1].copy_(st.tok)
        else:
            generated.append(int(st.tok[0]))
        if debug is not None:                                 # (tests): the logits, the draw and the token of generated token i, read back at once
            u = getattr(pick, "last_u", None)
            debug.append((st.logits[0].float().cpu(), None if u is None else float(u[0]), int(toks[i]) if captured else generated[-1]))

    def look(got, upto):
        ids = got.view(np.int64).tolist()
        hits = [i for i, t in enumerate(ids) if t in stop_ids]
        kept = hits[0] + 1 if hits else upto
        return kept, bool(hits), (ids[:kept], bool(hits), [hidden] + [hid_all[i:i + 1].view(1, 1, d) for i in range(kept - 1)])

    def loop_look(i):
        stopped = generated[-1] in stop_ids
        finished = stopped or len(generated) == max_new_tokens
        if finished:
            _raise_on_error_word(llm, cache, int(cache["err"][0]))
        return finished, (generated, stopped, hiddens)

    return types.SimpleNamespace(first=lambda logits: select(logits, 0), step=step, file=file, records=lambda upto: toks[:upto], look=look,
                                 loop_look=loop_look, reorder=None, counters=None, forward=None, needs_step=needs_step, debug=debug,
                                 n_dbg=len(debug) if debug is not None else 0, err_also="")


def _beam_policy(llm, cache, S, max_new_tokens, nb, scorer, eos_token_id, debug, captured):
    """The nb beams of one prompt as the rows of one step.  The step's record (cand_score | cand_index | next_scores | next_parent |
    next_tokens, one buffer) is the state the next step reads and is copied to a history row after every step; `scorer` (BeamScorer) replays
    the history on the host and says when the search is done.  Captured: the generated tail of the cache follows the chosen parents inside
    the step (ops.kv_permute_rows); in the loop the whole cache is re-ordered before it.  Yields nothing (None).  debug: a list that receives
    one dict per kept step."""
    cfg, dev = llm.cfg, llm.device
    d, V = cfg.hidden_size, cfg.vocab_size
    st = types.SimpleNamespace(logits=None)
    # the step record: one buffer, so that one copy files a step
    rec = torch.zeros(32 * nb, dtype=torch.uint8, device=dev)
    cs, ci = rec[:8 * nb].view(torch.float32), rec[8 * nb:16 * nb].view(torch.int32)
    ns, par, tok = rec[16 * nb:20 * nb].view(torch.float32), rec[20 * nb:24 * nb].view(torch.int32), rec[24 * nb:].view(torch.int64)
    hist = torch.empty((max_new_tokens, 32 * nb), dtype=torch.uint8, device=dev)
    first_scores = [0.0] + [-1e9] * (nb - 1)                  # HF's beam_scores[:, 1:] = -1e9: the first step ranks one row
    ns.copy_(torch.tensor(first_scores, dtype=torch.float32))
    scores_in = [torch.tensor(first_scores, dtype=torch.float32)]
    if captured:
        table, kept_alive = ops.kv_permute_table(cache)

    def unpack(row):
        """A history row on the host -> (cand_score, cand_index, next_scores, next_parent, next_tokens)."""
        return (row[:8 * nb].view(np.float32), row[8 * nb:16 * nb].view(np.int32), row[16 * nb:20 * nb].view(np.float32),
                row[20 * nb:24 * nb].view(np.int32), row[24 * nb:].view(np.int64))

    def feed(rows):
        """The scorer over recorded steps, until done -> done."""
        for row in rows:
            c_s, c_i, _, _, _ = unpack(row)
            if scorer.step([(float(s), int(i) // V, int(i) % V) for s, i in zip(c_s, c_i)]):
                return True
        return False

    def select(logits, shared=False):
        st.logits = logits
        ops.beam_topk(logits, ns, eos_token_id, cs, ci, ns, tok, par, cache["err"], nb=nb if shared else None)

    def first(logits):
        assert logits.shape[1] == V
        select(logits, shared=True)

    def step(forward, at):
        if captured:
            ops.kv_permute_rows(table, cache["k"][0], par, S, at[0:1], cache["err"])     # the tail follows the chosen parents
        emb = ops.splice_rows(llm.embed_tokens, None, tok if captured else tok.clone(), d)
        h = forward(emb.view(nb, 1, d))
        select(llm.next_token_logits(h.view(nb, d)))

    def reorder():
        if nb > 1:                                            # HF's _reorder_cache: the whole cache, by the chosen parents
            sel = par.to(torch.int64)
            cache["k"] = [t.index_select(0, sel) for t in cache["k"]]
            cache["v"] = [t.index_select(0, sel) for t in cache["v"]]

    def file(i):
        hist[i].copy_(rec)
        if debug is not None:                # (tests): this step's logits, input scores, candidates and selection, read back at once
            c_s, c_i, n_s, n_p, n_t = unpack(rec.cpu().numpy())
            debug.append({"logits": st.logits.float().cpu().expand(nb, -1), "scores_in": scores_in[0], "cand_score": c_s, "cand_index": c_i,
                          "next_scores": n_s, "next_parent": n_p, "next_tokens": n_t})
            scores_in[0] = torch.from_numpy(n_s.copy())

    def look(got, upto):
        done = feed(got.reshape(-1, 32 * nb))
        return scorer.steps, done, None

    def loop_look(i):
        row = hist[i:i + 1].cpu().numpy()
        _raise_on_error_word(llm, cache, int(cache["err"][0]), also=err_also)
        return feed(row) or i == max_new_tokens - 1, None

    err_also = ", or the beam selection ran out of candidates (NaN logits)"
    return types.SimpleNamespace(first=first, step=step, file=file, records=lambda upto: hist[scorer.steps:upto], look=look, loop_look=loop_look,
                                 reorder=reorder, counters=None, forward=None, needs_step=False, debug=debug,
                                 n_dbg=len(debug) if debug is not None else 0, err_also=err_also)


def _batch_policy(llm, hiddens0, cache, lengths, max_new_tokens, stop_ids, pick, debug, captured, row_limits=None, row_stop_ids=None):
    """The B prompts of a group as the rows of one step: row b sits at its own position lengths[b] + i and sees its own lengths[b] + i + 1 keys
    (decode_step with per-row state); the pick runs over the [B, V] logits; one record of B tokens per step.  At a look the host finds each
    row's first stop id: the call is done when every row has stopped or at max_new_tokens, and what a row computed past its stop is discarded.
    Yields ([generated ids so far per row], [stopped per row], [[hidden states of the prompt, of each fed token] per row]).  hiddens0: the
    prefill's hidden states per row.  debug: a list that receives (fp32 logits [B, V] on the host, the B tokens) per kept step — with the
    step's draws (fp32 [B] on the host) between the two when the pick draws (_RowsPick.last_u).
    row_limits / row_stop_ids: optionally a max_new_tokens (<= max_new_tokens, the largest of them) and a stop-id set per row, in place of
    the shared ones: a row is finished at its first stop id or at its own limit, what it computes afterwards is discarded, and the group is
    done when every row is finished."""
    d, dev, B = llm.cfg.hidden_size, llm.device, len(lengths)
    needs_step = getattr(pick, "needs_step", False)
    limits = [max_new_tokens] * B if row_limits is None else [int(n) for n in row_limits]
    stops = [stop_ids] * B if row_stop_ids is None else list(row_stop_ids)
    assert len(limits) == len(stops) == B and all(1 <= n <= max_new_tokens for n in limits)
    if getattr(pick, "err", False) is None:                   # a pick with an error word of its own to set (_RowsPick): the cache's
        pick.err = cache["err"]
    st = types.SimpleNamespace(tok=None, logits=None)        # the selected tokens (int64 [B] on the device) and the logits they came from
    generated, hiddens = [], []                               # the loop's record: [B] tokens on the host and [B, 1, d] hidden states per step
    if captured:
        toks = torch.empty((max_new_tokens, B), dtype=torch.int64, device=dev)
        hid_all = torch.empty((max_new_tokens, B, d), dtype=torch.bfloat16, device=dev)
        h_static = torch.empty((B, 1, d), dtype=torch.bfloat16, device=dev)

    def counters():
        """[position of the fed token per row | keys after appending it per row | the number of the token being generated]"""
        return torch.tensor(list(lengths) + [n + 1 for n in lengths] + [1], dtype=torch.int32, device=dev)

    def forward(emb, ctr, pass_dev):
        return llm.decode_step(emb, cache, None, pass_dev=pass_dev, rows=(ctr[:B], ctr[B:2 * B]))

    def select(logits, step_no):
        st.logits = logits
        tok = pick(logits, step_no)
        if captured and st.tok is not None:
            st.tok.copy_(tok)
        else:
            st.tok = tok

    def step(fwd, at):
        emb = ops.splice_rows(llm.embed_tokens, None, st.tok, d)
        h = fwd(emb.view(B, 1, d))
        if captured:
            h_static.copy_(h)
            select(llm.next_token_logits(h.view(B, d)), at[2 * B:2 * B + 1] if needs_step else None)
        else:
            hiddens.append(h)
            select(llm.next_token_logits(h.view(B, d)), at)

    def file(i):
        if captured:
            if i:
                hid_all[i - 1].copy_(h_static.view(B, d))
            toks[i].copy_(st.tok)
        else:
            generated.append(st.tok.cpu().numpy())
        if debug is not None:
            u = getattr(pick, "last_u", None)
            debug.append((st.logits.float().cpu(),) + (() if u is None else (u.cpu(),)) + ((toks[i] if captured else st.tok).tolist(),))

    def kept_rows(ids):
        """ids [n, B] on the host -> per row the steps kept (up to and including its first stop id, its limit at the most), whether it
        stopped, and whether it is finished (stopped, or at its limit)."""
        kept, stopped, finished = [], [], []
        for b in range(B):
            own = ids[:limits[b], b].tolist()
            hits = [i for i, t in enumerate(own) if t in stops[b]]
            kept.append(hits[0] + 1 if hits else len(own))
            stopped.append(bool(hits))
            finished.append(bool(hits) or len(own) == limits[b])
        return kept, stopped, finished

    def out_of(ids, kept, stopped, hidden_of):
        return ([ids[:kept[b], b].tolist() for b in range(B)], stopped,
                [[hiddens0[b]] + [hidden_of(i, b) for i in range(kept[b] - 1)] for b in range(B)])

    def look(got, upto):
        ids = got.view(np.int64).reshape(upto, B)
        kept, stopped, finished = kept_rows(ids)
        return max(kept), all(finished), out_of(ids, kept, stopped, lambda i, b: hid_all[i, b].view(1, 1, d))

    def loop_look(i):
        ids = np.stack(generated)
        kept, stopped, done = kept_rows(ids)
        finished = all(done) or len(generated) == max_new_tokens
        if finished:
            _raise_on_error_word(llm, cache, int(cache["err"][0]))
        return finished, out_of(ids, kept, stopped, lambda j, b: hiddens[j][b].view(1, 1, d))

    return types.SimpleNamespace(first=lambda logits: select(logits, 0), step=step, file=file, records=lambda upto: toks[:upto], look=look,
                                 loop_look=loop_look, reorder=None, counters=counters, forward=forward, needs_step=needs_step, debug=debug,
                                 n_dbg=len(debug) if debug is not None else 0, err_also="")


def _row_prompt(ids, images, attention_mask, kwargs, b):
    """Row b of a batch as one prompt -> (ids [1, L_b] without the row's padding, its CLIP images, its PromptExtras)."""
    row = ids[b:b + 1]
    if attention_mask is not None:
        row = row[:, _np_ids(attention_mask)[b].astype(bool)]               # drop this row's padding
    img = images[b] if isinstance(images, (list, tuple)) else images[b:b + 1]
    if isinstance(images, (list, tuple)):
        img = [img]
    rm, rv = kwargs.get("region_masks") or (), kwargs.get("valid_region_masks_bool") or ()
    if len(rm) > 0:            # the collator's flat list holds one entry per sample WITH regions: pick this row's
        before = sum(1 for v in rv[:b] if any(v))
        rm, rv = (rm[before:before + 1] if any(rv[b]) else ()), rv[b:b + 1]
    return row, img, PromptExtras(kwargs.get("mask_images"), kwargs.get("image_token_types"), kwargs.get("image_token_lengths"), rm, rv)


def _padded_rows(rows, eos_token_id):
    """Output rows (prompt + answer, int64 [L_b + n_b] each) -> int64 [B, max], right-padded with eos: HF generate's layout."""
    n = max(r.shape[0] for r in rows)
    return torch.from_numpy(np.stack([np.concatenate([r, np.full(n - r.shape[0], eos_token_id, np.int64)]) for r in rows]))


# ---------------------------------------------------------------------- the model's generation surface
class GenerationMixin:
    """The decode entry points of MedPLIBForCausalLM.  Expects of its host: config, device_, model.llm, seg_token_idx, decode_with_graph,
    train(), sync_side_streams(), adapters_merged(), _require_shadowable(), _encode_and_plan() and _seg_mask()."""

    @contextlib.contextmanager
    def _decoding(self, who):
        """The prologue and epilogue of a decode entry point: adapters under expert parallelism are refused before any state changes, the
        calling stream is ordered behind the side streams, the model is in eval mode and, with adapters attached, decodes on their shadow
        merge (adapters_merged()); leaving the block — also on an exception or when a generator is closed early — puts the plain weights
        and the mode back.  In 8-bit or 4-bit mode (enable_decode_8bit / enable_decode_4bit) the copies are re-quantised here, before anything is captured, when the parameters were
        written since they were made.  Yields the ExitStack that holds the merge: close() it to have the plain weights back before the block ends."""
        self._require_shadowable(who)
        self.sync_side_streams()
        self._refresh_decode_weights(who)
        was_training = self.training
        self.train(False)
        try:
            with contextlib.ExitStack() as merged:
                merged.enter_context(self.adapters_merged())
                yield merged
        finally:
            self.train(was_training)

    # ------------------------------------------------------------------ quantised decode weights (llama.DECODE_MODES): one helper set under the public pairs
    def _decode_bits_on(self, bits):
        """Whether the decode steps stream the copies of mode `bits`."""
        dw = self.model.llm.decode_weights
        return dw is not None and dw.mode.bits == bits

    def _enable_decode_weights(self, bits, on):
        """enable_decode_<bits>bit(on): off drops the copies only when this mode is the one that is on; on (re-)quantises, which drops the
        other mode's copies."""
        llm = self.model.llm
        if not on:
            if self._decode_bits_on(bits):
                llm.drop_decode_weights()
            return self
        self._refuse_in_shadow(f"enable_decode_{bits}bit")
        self.sync_side_streams()
        llm.quantize_decode_weights(bits)
        return self

    def _refresh_decode_weights(self, who):
        """The decode prologue's part in a quantised mode: what enabling it refuses may have been attached since (adapters, expert parallelism),
        and an optimizer step or a checkpoint load (ops.PARAM_EPOCH) leaves the copies stale."""
        llm = self.model.llm
        if llm.decode_weights is None:
            return
        mode = llm.decode_weights.mode
        why = llm.decode_weights_unsupported(mode.bits)
        if why is not None:
            raise NotImplementedError(f"{who}() in {mode.words} decode mode: {why} (or enable_decode_{mode.bits}bit(False))")
        if llm.decode_weights.epoch != ops.PARAM_EPOCH:
            llm.quantize_decode_weights(mode.bits)

    # ------------------------------------------------------------------ 8-bit decode weights (the reference worker's --load-8bit)
    @property
    def decode_8bit(self):
        """Whether the decode steps stream the 8-bit copies of the decoder projections."""
        return self._decode_bits_on(8)

    def enable_decode_8bit(self, on=True):
        """The reference worker's --load-8bit (model/serve/model_worker.py:72,100,642 -> builder.py:39, bitsandbytes) as a SPEED mode of the
        decode steps, not a memory mode: int8 copies of the decoder's qkv, o, gate|up and down projections (row-wise absmax, bitsandbytes'
        weight format; LlamaStack.quantize_decode_weights) are added beside the bf16 weights, and every single-token decode step of evaluate /
        generate / generate_sample / generate_beam / generate_stream — captured or looped — streams them: half the bytes per token.  Prefill,
        training and export keep the bf16 weights and their bits; lm_head, the embeddings, the norms and the MoE gate stay as they are; the
        activations stay bf16 (W8A16: no int8 activations, no outlier split).  NotImplementedError, with the mode left as it was, for top-2
        routing, the residual MoE, expert parallelism, attached adapters (merge_and_unload() first) and dimensions that are no multiple of 16.
        enable_decode_8bit(False) drops the copies: today's path, bit for bit.  Exclusive with enable_decode_4bit: enabling one mode drops the
        other's copies."""
        return self._enable_decode_weights(8, on)

    # ------------------------------------------------------------------ 4-bit NF4 decode weights (the reference's load_in_4bit, nf4)
    @property
    def decode_4bit(self):
        """Whether the decode steps stream the NF4 copies of the decoder projections."""
        return self._decode_bits_on(4)

    def enable_decode_4bit(self, on=True):
        """The reference's load_in_4bit with bnb_4bit_quant_type="nf4" (model/builder.py:41-47, chat.py:89-98; bitsandbytes) as a SPEED mode of
        the decode steps, like enable_decode_8bit and exclusive with it (enabling one drops the other's copies): NF4 copies of the decoder's
        qkv, o, gate|up and down projections — 4-bit codes into QLoRA's table with one fp32 absmax per 64 weights, 0.5625 bytes per weight
        (LlamaStack.quantize_decode_weights) — are added beside the bf16 weights, and every single-token decode step of evaluate / generate
        / generate_sample / generate_beam / generate_stream, captured or looped, streams them.  The absmax stays fp32 (no double
        quantisation), the table is NF4 only (no fp4), and the GEMV multiplies with the table rounded to bf16.  Prefill, training and export
        keep the bf16 weights and their bits; lm_head, the embeddings, the norms and the MoE gate stay as they are.  NotImplementedError, with
        the mode left as it was, for top-2 routing, the residual MoE, expert parallelism, attached adapters (merge_and_unload() first) and
        dimensions that are no multiple of 64.  enable_decode_4bit(False) drops the copies: today's path, bit for bit."""
        return self._enable_decode_weights(4, on)

    def _graph_decode_ok(self):
        """Whether the captured step computes what the token-by-token loop computes for this model: top-1, or top-2 on one rank without the
        residual MoE and without injected gate draws (a host-side provider would be frozen into the graph)."""
        cfg, llm = self.config, self.model.llm
        if cfg.top_k_experts == 1:
            return True
        return cfg.top_k_experts == 2 and llm.ep is None and not cfg.use_residual and llm.rts_uniform_provider is None

    def _captures(self, max_new_tokens):
        """Whether a call decodes through the captured graph (more than two tokens: one replay at least), else token by token."""
        return bool(self.decode_with_graph and max_new_tokens > 2 and self._graph_decode_ok())

    def _plan_embeds(self, ids, images_clip, extras):
        """One prompt planned and spliced -> (its input embeddings [1, S, d], S)."""
        cfg, dev, llm = self.config, self.device_, self.model.llm
        plan, feats = self._encode_and_plan(ids, None, None, images_clip, extras.mask_images, extras.image_token_types, extras.image_token_lengths,
                                            with_seg=False, region_masks=extras.region_masks if extras.region_masks else None,
                                            valid_region_masks_bool=extras.valid_region_masks_bool)
        src = _h2d(plan.src_code.reshape(-1), dev)
        S = plan.seq_len
        return ops.splice_rows(llm.embed_tokens, feats, src, cfg.hidden_size).view(1, S, cfg.hidden_size), S

    def _prefill_batch(self, prompts, max_new_tokens, batched=False):
        """The prompts of a batch group — (ids, images_clip, extras) each — planned first, then each prefilled at batch 1 (the bits of
        generate()'s prefill) into its own row of ONE KV cache of len(prompts) rows and max(S_b) + max_new_tokens positions, allocated before
        the first prefill so that the RoPE tables have grown before anything is captured.  -> ([hidden per row], cache, [S_b]).
        batched: the planned embeddings stacked, zero-padded on the right to max(S_b), through ONE LlamaStack.forward(seg_lens=[S_b]) into
        the group's cache — one pass over the weights for the group, every MoE layer routing each prompt as a pass of its own; the hidden
        states per row are views [1, S_b, d] of that pass's output.  The K/V the pad positions wrote are dead by construction: row b's first
        decode step appends at S_b, over the first of them, and the key count per row bounds every read, so no step ever reads a pad
        position's K/V.  A group of one takes the per-row path either way (the same launches)."""
        llm = self.model.llm
        planned = [self._plan_embeds(*p) for p in prompts]
        lengths = [S for _, S in planned]
        cache = llm.new_kv_cache(len(prompts), max(lengths) + max_new_tokens)
        if batched and len(prompts) > 1:
            embeds = torch.zeros((len(prompts), max(lengths), self.config.hidden_size), dtype=planned[0][0].dtype, device=self.device_)
            for b, (row, S) in enumerate(planned):
                embeds[b, :S].copy_(row[0])
            hidden = llm.forward(embeds, None, kv_cache=cache, seg_lens=lengths)[0]
            return [hidden[b:b + 1, :S] for b, S in enumerate(lengths)], cache, lengths
        hiddens = []
        for b, (embeds, S) in enumerate(planned):
            row = {"len": 0, "k": [t[b:b + 1] for t in cache["k"]], "v": [t[b:b + 1] for t in cache["v"]], "err": cache["err"]}
            hiddens.append(llm.forward(embeds, None, kv_cache=row)[0])
        cache["len"] = max(lengths)
        return hiddens, cache, lengths

    def _prefill(self, ids, images_clip, extras, max_new_tokens, rows=1):
        """The spliced prompt through the stack at batch 1, into row 0 of a KV cache of `rows` rows and S + max_new_tokens positions (allocated
        here, so the RoPE tables have grown before anything is captured); the prompt's K/V copied to the other rows.  -> (hidden, cache, S)."""
        llm = self.model.llm
        embeds, S = self._plan_embeds(ids, images_clip, extras)
        cache = llm.new_kv_cache(rows, S + max_new_tokens)
        row0 = cache if rows == 1 else {"len": 0, "k": [t[:1] for t in cache["k"]], "v": [t[:1] for t in cache["v"]], "err": cache["err"]}
        hidden, _, _ = llm.forward(embeds, None, kv_cache=row0)
        cache["len"] = S
        for t in (cache["k"] + cache["v"] if rows > 1 else ()):
            t[1:, :S].copy_(t[:1, :S])
        return hidden, cache, S

    def _drive(self, policy, hidden, cache, S, max_new_tokens, captured, looks=None):
        """The steps of one call after its prefill: step 0 from the prefill's last position (hidden [1, S, d]; a batch group: the rows' last
        positions [B, d]), then the captured graph or the loop.  A generator of what the policy yields: at `looks` (default: _default_looks)
        when captured, after every token in the loop."""
        llm = self.model.llm
        policy.first(llm.next_token_logits(hidden[0, -1:] if hidden.dim() == 3 else hidden))
        policy.file(0)
        self.last_decode_path = "graph" if captured else "loop"
        if captured:
            yield from _captured_steps(llm, cache, S, policy, looks if looks is not None else _default_looks(max_new_tokens))
        else:
            yield from _loop_steps(llm, cache, policy, max_new_tokens)

    def _decode(self, ids, images_clip, max_new_tokens, stop_ids, extras=NO_EXTRAS, pick=_argmax_pick, looks=None, host_pick=False, debug=None):
        """Prefill of the spliced prompt, then single-token decode steps against the KV cache, the next token chosen by `pick` (the greedy
        argmax unless told otherwise), until one of `stop_ids` or max_new_tokens.  Through the captured graph when the model allows it
        (_captures) and the pick runs on the device (not host_pick), else token by token.  A generator of (generated ids so far, stopped,
        [hidden states of the prompt, of each fed token]): the graph path yields at `looks`, the loop after every token."""
        hidden, cache, S = self._prefill(ids, images_clip, extras, max_new_tokens)
        captured = self._captures(max_new_tokens) and not host_pick
        policy = _single_row_policy(self.model.llm, hidden, cache, max_new_tokens, stop_ids, pick, debug, captured)
        yield from self._drive(policy, hidden, cache, S, max_new_tokens, captured, looks)

    def _decode_batch(self, prompts, max_new_tokens, stop_ids, pick=_argmax_pick, looks=None, debug=None, row_limits=None, row_stop_ids=None,
                      batch_prefill=False):
        """_decode for the prompts of one batch group, (ids, images_clip, extras) each, as the rows of one decode step (_batch_policy): every
        prompt prefilled at batch 1 into its row of one cache, then single-token steps at B rows with a position and a key count per row,
        the next tokens chosen by `pick` over the [B, V] logits.  Through the captured graph under _decode's conditions, else token by token.
        A generator of ([generated ids so far per row], [stopped per row], [[hidden states of the prompt, of each fed token] per row]).
        row_limits / row_stop_ids: a max_new_tokens and a stop-id set per row (_batch_policy).  batch_prefill: the group's prompts through one
        padded pass instead of a prefill per row (_prefill_batch(batched=True))."""
        hiddens, cache, lengths = self._prefill_batch(prompts, max_new_tokens, batched=batch_prefill)
        captured = self._captures(max_new_tokens)
        policy = _batch_policy(self.model.llm, hiddens, cache, lengths, max_new_tokens, stop_ids, pick, debug, captured, row_limits, row_stop_ids)
        last = torch.cat([h[0, -1:] for h in hiddens])
        yield from self._drive(policy, last, cache, lengths, max_new_tokens, captured, looks)      # (S: the error message's positions, per row)

    def _greedy(self, ids, images_clip, max_new_tokens, eos_token_id, extras=NO_EXTRAS, pick=_argmax_pick):
        """HF `generate(do_sample=False, use_cache=True)` on one sample (MedPLIB.py:592-606; prepare_inputs_for_generation,
        medplib_moe_llama.py:451-485): prefill of the spliced prompt, then single-token decode steps against the KV cache (_decode).
        Returns (output_ids [1, L + n] on the host, [hidden states of the prompt, of each fed token])."""
        generated, hiddens = [], []
        for generated, _, hiddens in self._decode(ids, images_clip, max_new_tokens, (eos_token_id,), extras, pick=pick):
            pass
        return np.concatenate([ids, np.asarray(generated, dtype=np.int64)[None]], 1), list(hiddens)

    def _beam_row(self, ids, images_clip, max_new_tokens, eos_token_id, nb, length_penalty, early_stopping, extras, debug):
        """Beam search on one sample -> (generated ids of the winning hypothesis, its score): the prefill of _decode into a cache of nb rows,
        then one decode step per token at B = nb (_beam_policy)."""
        from ..beam import BeamScorer
        hidden, cache, S = self._prefill(ids, images_clip, extras, max_new_tokens, rows=nb)
        scorer = BeamScorer(nb, length_penalty, early_stopping, eos_token_id, length_base=ids.shape[1], max_new_tokens=max_new_tokens)
        captured = self._captures(max_new_tokens)
        policy = _beam_policy(self.model.llm, cache, S, max_new_tokens, nb, scorer, eos_token_id, debug, captured)
        for _ in self._drive(policy, hidden, cache, S, max_new_tokens, captured):
            pass
        return scorer.finalize()

    def _generate_rows(self, who, input_ids, images, attention_mask, max_new_tokens, eos_token_id, kwargs, decode_row):
        """generate() / generate_sample() / generate_beam(): batch rows decoded one after the other by decode_row(b, row ids, images,
        PromptExtras) -> ids [1, L + n]; output ids [B, L + n_max], prompt included, right-padded with eos."""
        ids = _np_ids(input_ids).astype(np.int64)
        rows = []
        with self._decoding(who):
            for b in range(ids.shape[0]):
                rows.append(decode_row(b, *_row_prompt(ids, images, attention_mask, kwargs, b))[0])
        return _padded_rows(rows, eos_token_id)

    @torch.no_grad()
    def generate(self, input_ids, images=None, attention_mask=None, max_new_tokens=512, eos_token_id=2, **kwargs):
        """The VQA entry the drivers use (`model.generate(input_ids, images=images_clip, attention_mask=..., max_new_tokens=...,
        do_sample=False)`, vqa_infer.py:430-442): greedy decoding, one sample per call like the reference's loop (batch rows are
        decoded one after the other).  Returns output ids [B, L + n_max] (right-padded with eos), prompt included, as HF does.
        HF generate kwargs the reference driver passes are accepted when they mean greedy decoding and refused loudly otherwise:
        sampling is generate_sample(), beam search generate_beam()."""
        _check_kwargs("generate", kwargs)
        return self._generate_rows("generate", input_ids, images, attention_mask, max_new_tokens, eos_token_id, kwargs,
                                   lambda b, row, img, extras: self._greedy(row, img, max_new_tokens, eos_token_id, extras)[0])

    @torch.no_grad()
    def generate_batch(self, input_ids, images=None, attention_mask=None, max_new_tokens=512, eos_token_id=2, batch_rows=8, batch_prefill=False,
                       **kwargs):
        """generate() with the prompts decoded TOGETHER: the rows are taken in groups of `batch_rows` (1..8, else ValueError) and the prompts
        of a group — whatever their lengths — are the rows of one decode step, so a group pays one pass over the decoder weights per token
        instead of one per prompt (_decode_batch, _batch_policy).  Each prompt is prefilled at batch 1 as in generate(); a row stops at its
        own eos (what the step computes for it afterwards is discarded) and a group is done when every row has stopped or at max_new_tokens.
        A MoE layer routes every row as generate() does (capacity = the rows of the group, no draws): no row is dropped because of its
        batch-mates, so a row's answer does not depend on the others; the rows of a top-1 layer that name the same expert share one pass over its
        weights — bf16, or the int8 / NF4 copies of the quantised mode that is on (ops.gemv_grouped, ops.gemv_grouped_w8 / _w4: the indexed
        forms' bits), and so do the (row, choice) entries of a top-2 layer on the bf16 weights (ops.gemv_grouped_top2_gate_up / _down: the
        per-entry pair's bits, at most min(E, 2 rows) expert MLPs read instead of 2 rows); it is generate()'s function in another summation order (the narrow
        projections of one row take the K-split form, of several the shared one), not its bits.  Same return layout as generate(): prompt
        included, right-padded with eos.  batch_rows = 8: the shared GEMV reads the weights once for up to four rows and twice for five to
        eight, and eight rows still gave more tokens per second than four on the dense and on the MoE model at 7B (profiles/batch_decode.md:
        +10 % and +13 %; four rows are the better latency).  Refused: sampling (generate_sample) and beams (generate_beam) per row, and — NotImplementedError
        before any state changes — gate sampling or an injected draw provider, the residual MoE and expert parallelism.
        batch_prefill=True (off by default): a group of two or more prompts is prefilled as ONE pass over the prompts right-padded to the
        longest (_prefill_batch(batched=True), LlamaStack.forward(seg_lens=)) instead of one pass per prompt.  A MoE layer of that pass routes
        every prompt as a pass of its own, at the capacity of its own length (ops.moe_route_top1_segments / _top2_segments): the experts, the
        dropped tokens and the slot order of a prompt are those of its batch-1 prefill on the same gate values, whoever its batch-mates are.
        The GEMMs see other row counts than at batch 1, so a row is the per-row prefill's function in another summation order, not its bits.
        Not built: evaluate() / <SEG> masks per batch."""
        _check_kwargs("generate_batch", kwargs)
        n_rows, max_new_tokens = int(batch_rows), int(max_new_tokens)
        if not 1 <= n_rows <= 8:
            raise ValueError(f"generate_batch(): batch_rows={batch_rows} must lie in 1..8 (the rows of one decode step)")
        assert max_new_tokens >= 1
        why = self.model.llm.batch_rows_unsupported()
        if why is not None:
            raise NotImplementedError(f"generate_batch(): {why}: call generate()")
        return self._generate_groups(input_ids, images, attention_mask, max_new_tokens, eos_token_id, n_rows, kwargs, _argmax_pick,
                                     batch_prefill=batch_prefill)

    @torch.no_grad()
    def _generate_groups(self, input_ids, images, attention_mask, max_new_tokens, eos_token_id, n_rows, kwargs, pick, pick_of_group=None,
                         who="generate_batch", debug=None, batch_prefill=False):
        """generate_batch() behind its argument checks: the rows in groups of n_rows through _decode_batch, the next tokens chosen by
        pick(logits [B, V], step) -> int64 [B] — or, with pick_of_group(first row, rows) -> pick, by a pick made for each group (the rows'
        own sampling parameters); output ids [B, L + n_max], prompt included, right-padded with eos.  batch_prefill: _decode_batch's."""
        ids = _np_ids(input_ids).astype(np.int64)
        rows = []
        with self._decoding(who):
            prompts = [_row_prompt(ids, images, attention_mask, kwargs, b) for b in range(ids.shape[0])]
            for g0 in range(0, len(prompts), n_rows):
                group = prompts[g0:g0 + n_rows]
                generated = [[] for _ in group]
                if pick_of_group is not None:
                    pick = pick_of_group(g0, len(group))
                # (closed before the prologue is undone: the driver's `finally` settles the pass counter)
                with contextlib.closing(self._decode_batch(group, max_new_tokens, (eos_token_id,), pick=pick, debug=debug,
                                                           batch_prefill=batch_prefill)) as steps:
                    for generated, _, _ in steps:
                        pass
                rows += [np.concatenate([p[0][0], np.asarray(g, dtype=np.int64)]) for p, g in zip(group, generated)]
        return _padded_rows(rows, eos_token_id)

    @torch.no_grad()
    def generate_sample(self, input_ids, images=None, attention_mask=None, max_new_tokens=512, eos_token_id=2, temperature=1.0, top_k=50,
                        top_p=1.0, sample_seed=None, **kwargs):
        """generate() with HF's do_sample=True (what vqa_infer.py:430-442 asks for with --temperature > 0): every next token is drawn from
        softmax(logits / temperature) truncated by top-k, then top-p (HF 4.31's TemperatureLogitsWarper -> TopKLogitsWarper ->
        TopPLogitsWarper; top_k = 50 is its GenerationConfig default, top_p=None means 1.0), by inverse CDF at the keyed generator's
        uniforms (_SamplePick, ops.sample_rows_filtered): HF's distribution, not torch.multinomial's draws.  Row b draws under seed
        sample_seed + b; sample_seed=None takes one from torch's global generator, as the serving worker does, so torch.manual_seed makes
        a run repeatable.  Same return layout as generate(): prompt included, right-padded with eos.  temperature <= 0 raises ValueError
        as HF does; beam search and repetition penalty are not built."""
        if not float(temperature) > 0:
            raise ValueError(f"generate_sample(): temperature={temperature} has to be a strictly positive float (greedy decoding: generate())")
        _check_kwargs("generate_sample", kwargs)
        if kwargs.get("do_sample") is False:
            raise ValueError("generate_sample(): do_sample=False asks for greedy decoding: call generate()")
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,))) if sample_seed is None else int(sample_seed)
        top_k, top_p = int(top_k or 0), 1.0 if top_p is None else float(top_p)

        def decode_row(b, row, img, extras):
            pick = _SamplePick(temperature, seed + b, self.device_, top_k=top_k, top_p=top_p)
            return self._greedy(row, img, max_new_tokens, eos_token_id, extras, pick=pick)[0]

        return self._generate_rows("generate_sample", input_ids, images, attention_mask, max_new_tokens, eos_token_id, kwargs, decode_row)

    @torch.no_grad()
    def generate_sample_batch(self, input_ids, images=None, attention_mask=None, max_new_tokens=512, eos_token_id=2, temperature=1.0, top_k=50,
                              top_p=1.0, sample_seed=None, batch_rows=8, **kwargs):
        """generate_sample() with the rows decoded TOGETHER, as generate_batch() decodes generate()'s: the rows are taken in groups of
        `batch_rows` (1..8, else ValueError) and a group is the rows of one decode step, drawn and picked by one launch each (_RowsPick:
        ops.sample_uniform_rows, ops.pick_rows).  temperature, top_k and top_p are scalars or one value per row (a sequence of another length:
        ValueError), so rows of one step may sample differently; row b draws under sample_seed + b, generate_sample()'s rule, and
        sample_seed=None takes a seed from torch's global generator.  Same return layout: prompt included, right-padded with eos.
        A row is generate_sample()'s function in another summation order, as a generate_batch row is generate()'s — not its tokens.  What IS
        exact: token i of row b is the single-row op (ops.sample_rows / ops.sample_rows_filtered, by generate_sample()'s rule) on that step's
        own logits row at the draw for (sample_seed + b, i).  ValueError for a temperature that is not > 0 and for do_sample=False;
        NotImplementedError, before any state changes, for beams and wherever generate_batch() refuses the model (gate sampling or an
        injected draw provider, the residual MoE, expert parallelism).  batch_prefill=True (a keyword, off by default): generate_batch()'s
        switch, one padded prefill pass per group.  debug: a list that receives (fp32 logits [B, V], u [B], tokens [B])
        per kept step of every group (tests; costs a sync per token)."""
        debug, batch_prefill = kwargs.pop("debug", None), bool(kwargs.pop("batch_prefill", False))
        n_prompts = int(_np_ids(input_ids).shape[0])

        def per_row(value, name, cast):
            if isinstance(value, (list, tuple, np.ndarray)) or torch.is_tensor(value):
                if len(value) != n_prompts:
                    raise ValueError(f"generate_sample_batch(): {name} has {len(value)} entries for {n_prompts} rows (a scalar, or one per row)")
                return [cast(v) for v in value]
            return [cast(value)] * n_prompts

        temperatures = per_row(temperature, "temperature", float)
        top_ks = per_row(top_k, "top_k", lambda k: int(k or 0))
        top_ps = per_row(top_p, "top_p", lambda p: 1.0 if p is None else float(p))
        for t in temperatures:
            if not t > 0:
                raise ValueError(f"generate_sample_batch(): temperature={t} has to be a strictly positive float (greedy decoding: generate_batch())")
        _check_kwargs("generate_sample_batch", kwargs)
        if kwargs.get("do_sample") is False:
            raise ValueError("generate_sample_batch(): do_sample=False asks for greedy decoding: call generate_batch()")
        n_rows, max_new_tokens = int(batch_rows), int(max_new_tokens)
        if not 1 <= n_rows <= 8:
            raise ValueError(f"generate_sample_batch(): batch_rows={batch_rows} must lie in 1..8 (the rows of one decode step)")
        assert max_new_tokens >= 1
        why = self.model.llm.batch_rows_unsupported()
        if why is not None:
            raise NotImplementedError(f"generate_sample_batch(): {why}: call generate_sample()")
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,))) if sample_seed is None else int(sample_seed)

        def pick_of_group(g0, n):
            rows = slice(g0, g0 + n)
            return _RowsPick(temperatures[rows], top_ks[rows], top_ps[rows], [seed + b for b in range(g0, g0 + n)], self.device_)

        return self._generate_groups(input_ids, images, attention_mask, max_new_tokens, eos_token_id, n_rows, kwargs, None,
                                     pick_of_group=pick_of_group, who="generate_sample_batch", debug=debug, batch_prefill=batch_prefill)

    @torch.no_grad()
    def generate_beam(self, input_ids, images=None, attention_mask=None, max_new_tokens=512, eos_token_id=2, num_beams=4, length_penalty=1.0,
                      early_stopping=False, debug=None, **kwargs):
        """generate() with HF 4.31's beam search (GenerationMixin.beam_search + BeamSearchScorer; what vqa_infer.py:430-442 asks for with
        --num_beams > 1): generate(num_beams=, do_sample=False, num_return_sequences=1, length_penalty=, early_stopping=False | True), one
        sample at a time.  The num_beams beams of a prompt are the rows of one decode step: they share the position counter and one pass over
        the weights.  Between two steps the device ranks the candidates (ops.beam_topk) and re-orders the generated tail of the KV cache by
        the chosen parents (ops.kv_permute_rows); the hypotheses live on the host (medplib_amd.beam.BeamScorer, replayed over the recorded
        candidates at every look).  Decode path (last_decode_path): the captured graph under generate()'s conditions, else a token-by-token
        loop that re-orders the whole cache with index_select.  Same return layout as generate(): prompt included, right-padded with eos; an
        answer that ended on eos carries it when it fits, as HF's finalize writes it.  last_beam_scores: the winner's score per row.
        Refused: do_sample=True (beam sampling), num_return_sequences != 1, early_stopping="never", num_beams > 8.
        debug: a list that receives one dict per kept step — the fp32 logits [num_beams, V] on the host, the input beam scores, the candidates
        and the selection (tests; costs a sync per token)."""
        _check_kwargs("generate_beam", kwargs, ("num_return_sequences",))
        if (kwargs.get("num_return_sequences") or 1) != 1:
            raise NotImplementedError("generate_beam(): num_return_sequences != 1 is not built: the best beam is returned")
        if early_stopping not in (False, True):
            raise NotImplementedError(f"generate_beam(): early_stopping={early_stopping!r} is not built (False or True)")
        nb = int(num_beams)
        if not 1 <= nb <= 8:
            raise NotImplementedError(f"generate_beam(): num_beams={num_beams} is not built: 1 to 8 beams share one decode step")
        max_new_tokens = int(max_new_tokens)
        assert max_new_tokens >= 1
        self.last_beam_scores = []

        def decode_row(b, row, img, extras):
            new, score = self._beam_row(row, img, max_new_tokens, int(eos_token_id), nb, float(length_penalty), bool(early_stopping), extras, debug)
            self.last_beam_scores.append(score)
            return np.concatenate([row, np.asarray(new, dtype=np.int64)[None]], 1)

        return self._generate_rows("generate_beam", input_ids, images, attention_mask, max_new_tokens, eos_token_id, kwargs, decode_row)

    @torch.no_grad()
    def generate_stream(self, input_ids, images_clip, images=None, temperature=1.0, top_p=1.0, max_new_tokens=256, stop_token_id=None,
                        eos_token_id=2, stream_interval=1, sample_seed=0, resize_list=None, original_size_list=None, region_masks=(),
                        valid_region_masks_bool=(), attention_mask=None, uniforms=None, debug=None, stop_check=None, top_k=0, apply_top_p=False):
        """The serving worker's token loop (model/serve/model_worker.py generate_stream) on one sample, as a generator: prefill, then one
        decode step per token, yielding (new token ids so far, stopped, pred_mask) after tokens i with i % stream_interval == 0, after the
        last one (i == max_new_tokens - 1) and at a stop (eos_token_id, stop_token_id, or stop_check(ids) -> True at a yield: the worker's
        stop string).  Every yield's ids are a prefix of the next one's.

        temperature < 1e-4: greedy, the tokens of generate().  Otherwise token i is drawn from softmax(logits / temperature) by inverse CDF
        (ops.sample_rows) at the uniform the keyed generator gives for (sample_seed, i) (ops.sample_uniform): one seed, one answer; the
        stream matches torch.multinomial in distribution, not draw by draw.  apply_top_p=False (the default): top_p is accepted and
        IGNORED, as is top_k — the reference's worker reads top_p from the request and never uses it.  apply_top_p=True: the distribution
        is truncated before the draw by top_k (0: none), then top_p, as HF's warpers do (ops.sample_rows_filtered), in the loop and in the
        captured step alike.
        Decode path (last_decode_path): the captured graph when decode_with_graph and _graph_decode_ok() hold, max_new_tokens > 2 and no
        `uniforms` is injected; the draw and the pick are then part of the captured step, and the host looks at the ids (and the cache's error
        word) only at the yields.  Otherwise the token-by-token loop.  uniforms(i) -> float replaces the generator (tests); it runs on the
        host, so it forces the loop.
        pred_mask is None except in the stopping yield (an answer that runs into max_new_tokens gets none, as in the reference), and
        there only when `images` (the SAM input, with resize_list and original_size_list as in evaluate()) was given and a generated id
        is seg_token_idx: evaluate()'s mask of the first <SEG>.
        debug: a list that receives (fp32 logits row on the host, u or None, token) for every kept token (tests; costs a sync per token)."""
        with self._decoding("generate_stream"):              # (a generator: the shadow merge of attached adapters lives as long as it does)
            ids = _np_ids(input_ids).astype(np.int64)
            assert ids.shape[0] == 1, "generate_stream() decodes one sample, like the reference's worker"
            if attention_mask is not None:
                ids = ids[:, _np_ids(attention_mask)[0].astype(bool)]
            max_new_tokens, every = int(max_new_tokens), max(1, int(stream_interval))
            assert max_new_tokens >= 1
            if temperature < 1e-4:
                pick = _argmax_pick
            elif apply_top_p:
                pick = _SamplePick(temperature, sample_seed, self.device_, uniforms, top_k=top_k, top_p=1.0 if top_p is None else top_p)
            else:
                pick = _SamplePick(temperature, sample_seed, self.device_, uniforms)
            stop_ids = {int(t) for t in (eos_token_id, stop_token_id) if t is not None}
            due = lambda i: i % every == 0 or i == max_new_tokens - 1            # noqa: E731  the reference's condition on the token number
            looks = [i + 1 for i in range(max_new_tokens) if due(i)]
            extras = PromptExtras(region_masks=region_masks, valid_region_masks_bool=valid_region_masks_bool)
            # closed before the prologue is undone, also when the consumer stops reading early: the driver's `finally` settles the pass counter
            with contextlib.closing(self._decode(ids, images_clip, max_new_tokens, stop_ids, extras, pick=pick, looks=looks,
                                                 host_pick=uniforms is not None, debug=debug)) as steps:
                for generated, stopped, hiddens in steps:
                    i = len(generated) - 1
                    if not (stopped or due(i)):
                        continue
                    new = list(generated)
                    if not stopped and stop_check is not None and stop_check(new):
                        stopped = True
                    pred_mask = None
                    if stopped and images is not None and self.seg_token_idx in new:
                        output_ids = np.concatenate([ids, np.asarray(new, dtype=np.int64)[None]], 1)
                        pred_mask = self._seg_mask(output_ids, list(hiddens), images, resize_list, original_size_list)[0]
                    yield new, stopped, pred_mask
                    if stopped or i == max_new_tokens - 1:
                        break

    def generate_stream_batch(self, requests, stream_interval=1, eos_token_id=2, debug=None):
        """generate_stream() for 1 to 8 requests (StreamRequest; more: ValueError) as the rows of ONE decode step: the group pays one pass
        over the decoder weights per token, and every row is drawn and picked at its own request's parameters by one launch each (_RowsPick).
        Per request the meaning is generate_stream()'s: temperature < 1e-4 is greedy, top_p and top_k count only with apply_top_p, and the
        request stops at eos_token_id, at its stop_token_id, or when its stop_check(ids) is true at a yield.
        A generator of (row, new token ids so far, stopped, pred_mask): row r yields after its tokens i with i % stream_interval == 0, after
        its own last token (i == its max_new_tokens - 1) and at its stop; every yield's ids are a prefix of the row's next one, and nothing
        is yielded for a row after it has finished.  The group ends when every row has.  pred_mask is _seg_mask on that row's own ids and
        hidden states and appears only in its stopping yield, under generate_stream()'s conditions (the request has `images`, a generated id
        is seg_token_idx; an answer that runs into its limit gets none).
        Decode path (last_decode_path): the captured graph under generate_batch()'s conditions, else the loop; the host looks at the ids every
        stream_interval steps (and at the rows' last tokens).  A row is generate_stream()'s function in another summation order; exact is what
        generate_sample_batch() states: every token is the single-row op on its step's own logits row at the draw for (sample_seed, i).
        `uniforms` injection is not offered.  self.stream_batch_prefill = True (an attribute of the model beside decode_with_graph, off by
        default; this method's arguments are the worker's) is generate_batch()'s batch_prefill for the groups served here: one padded prefill
        pass for the group, so the time to the group's first token is one pass, not the sum of the rows' prefills.  NotImplementedError, before any state changes, wherever generate_batch() refuses the model.
        debug: a list that receives (fp32 logits [B, V], u [B], tokens [B]) per kept step (tests; costs a sync per token)."""
        requests = list(requests)
        if not 1 <= len(requests) <= 8:
            raise ValueError(f"generate_stream_batch(): {len(requests)} requests: 1 to 8 are the rows of one decode step")
        why = self.model.llm.batch_rows_unsupported()
        if why is not None:
            raise NotImplementedError(f"generate_stream_batch(): {why}: call generate_stream() per request")
        limits = [int(r.max_new_tokens) for r in requests]
        assert min(limits) >= 1
        greedy = [r.temperature < 1e-4 for r in requests]
        filtered = [r.apply_top_p and not g for r, g in zip(requests, greedy)]
        pick = _RowsPick([None if g else r.temperature for r, g in zip(requests, greedy)],
                         [int(r.top_k or 0) if f else 0 for r, f in zip(requests, filtered)],
                         [(1.0 if r.top_p is None else float(r.top_p)) if f else 1.0 for r, f in zip(requests, filtered)],
                         [r.sample_seed for r in requests], self.device_)
        return self._stream_batch(requests, limits, pick, max(1, int(stream_interval)), eos_token_id, debug, bool(self.stream_batch_prefill))

    @torch.no_grad()
    def _stream_batch(self, requests, limits, pick, every, eos_token_id, debug, batch_prefill=False):
        """generate_stream_batch() behind its argument checks."""
        with self._decoding("generate_stream_batch"):
            B, n_max = len(requests), max(limits)
            prompts, stops = [], []
            for r in requests:
                ids = _np_ids(r.input_ids).astype(np.int64)
                assert ids.shape[0] == 1, "a StreamRequest holds one sample"
                prompts.append((ids, r.images_clip, PromptExtras(region_masks=r.region_masks, valid_region_masks_bool=r.valid_region_masks_bool)))
                stops.append({int(t) for t in (eos_token_id, r.stop_token_id) if t is not None})
            due = lambda i, b: i % every == 0 or i == limits[b] - 1            # noqa: E731  generate_stream's condition, on the row's own limit
            looks = sorted({i + 1 for i in range(n_max) if i % every == 0} | set(limits))
            finished, sent = [False] * B, [0] * B
            with contextlib.closing(self._decode_batch(prompts, n_max, (), pick=pick, looks=looks, debug=debug, row_limits=limits,
                                                       row_stop_ids=stops, batch_prefill=batch_prefill)) as steps:
                for generated, stopped_rows, hiddens in steps:
                    for b, r in enumerate(requests):
                        new = list(generated[b])
                        i, stopped = len(new) - 1, stopped_rows[b]
                        if finished[b] or len(new) == sent[b] or not (stopped or due(i, b)):
                            continue
                        sent[b] = len(new)
                        if not stopped and r.stop_check is not None and r.stop_check(new):
                            stopped = True
                        pred_mask = None
                        if stopped and r.images is not None and self.seg_token_idx in new:
                            output_ids = np.concatenate([prompts[b][0], np.asarray(new, dtype=np.int64)[None]], 1)
                            pred_mask = self._seg_mask(output_ids, list(hiddens[b]), r.images, r.resize_list, r.original_size_list)[0]
                        finished[b] = stopped or i == limits[b] - 1
                        yield b, new, stopped, pred_mask
                    if all(finished):
                        break

    # ------------------------------------------------------------------ evaluate (MedPLIB.py:574-680)
    @torch.no_grad()
    def evaluate(self, images_clip, images, input_ids, resize_list, original_size_list, region_masks=(), valid_region_masks_bool=(),
                 max_new_tokens=512, tokenizer=None, attention_mask=None, inference_demo=False, mask_images=None,
                 image_token_types=None, image_token_lengths=None, eos_token_id=2):
        """Greedy generation with a KV cache (prefill + single-token decode steps), then one mask per sample from the hidden
        state that predicts the first <SEG> (or position -2 when no <SEG> was generated) — MedPLIB.py:574-680.
        Returns (output_ids [1, L + n_generated] int64 on the host, [pred_mask [1,H,W]]).

        Reference quirk kept: the concatenated per-step hidden states cover the spliced prompt and the first n-1 generated
        tokens (the last generated token is never fed back), i.e. one position FEWER than build_seg_token_mask(output_ids)
        yields; the mask's final position is always False (shifted mask), so it is truncated to the hidden length."""
        with self._decoding("evaluate") as merged:
            ids = _np_ids(input_ids).astype(np.int64)
            assert ids.shape[0] == 1, "evaluate() decodes one sample at a time, like the reference's validate_seg (vqa_infer.py:528)"
            extras = PromptExtras(mask_images, image_token_types, image_token_lengths, region_masks, valid_region_masks_bool)
            output_ids, hiddens = self._greedy(ids, images_clip, max_new_tokens, eos_token_id, extras)
            merged.close()                               # the mask tail reads no decoder weight: the plain weights are back before it
            if (output_ids[:, 1:] == self.seg_token_idx).sum() == 0 and inference_demo:
                return torch.from_numpy(output_ids), []
            return torch.from_numpy(output_ids), self._seg_mask(output_ids, hiddens, images, resize_list, original_size_list, image_token_lengths)
