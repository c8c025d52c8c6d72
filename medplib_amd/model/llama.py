"""Llama-7B decoder stack (dense or DeepSpeed-style MoE MLPs) over the HIP kernels.

Mirrors `MoELlamaModel_forward` / `MoELlamaDecoderLayer_forward` (model/medplib/model/language_model/
medplib_moe_llama.py:110-305) and HF-4.31 LlamaAttention/LlamaMLP/LlamaRMSNorm:
    x = x + o_proj(attn(rope(q), rope(k), v));  x = x + mlp(rmsnorm(x))   with mlp = SwiGLU or MoE(top-1 experts).
Weights are held in kernel layout (fused qkv [3d,d], gate/up fused [2ff,d] with rows interleaved in blocks of 32 for the
SwiGLU-in-epilogue GEMM, experts stacked [E,...]) and are
imported from / exported to the HF checkpoint key layout by load_hf / export_hf."""
import collections
import math
import os

import torch

from .. import ops


def _rope_tables(seq, head_dim, theta, device, start=0):
    """cos / sin [seq - start, head_dim / 2] fp32 of positions start .. seq - 1 (HF 4.31 LlamaRotaryEmbedding's fp32 formula)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    freqs = torch.outer(torch.arange(start, seq, dtype=torch.float32), inv)
    return freqs.cos().contiguous().to(device), freqs.sin().contiguous().to(device)


# MP_GEMV_GROUPED=0: the ragged batch rows of a MoE layer keep the indexed (top-2: per-entry) expert GEMVs (one weight stream per row or entry)
# instead of the grouped form (one per expert): an A/B switch, read once; LlamaStack.group_expert_gemvs starts from it
GEMV_GROUPED = os.environ.get("MP_GEMV_GROUPED", "1") != "0"

ROPE_GROW_ROWS = 1024     # RoPE tables grow in whole multiples of this many rows (slowly lengthening prompts do not reallocate each call)


def rope_rows_for(n, rows):
    """Rows a RoPE table of `rows` rows must have to cover positions 0 .. n - 1: unchanged when it does, else n rounded up to ROPE_GROW_ROWS."""
    return rows if n <= rows else -(-n // ROPE_GROW_ROWS) * ROPE_GROW_ROWS


# THE table of quantised decode modes, keyed by bit width: what a decode row streams in place of the bf16 weights.  words: the mode in messages;
# quantizer / gemv: NAMES of ops functions, resolved at call time (tests count calls by patching them on the module); multiple / why: what
# hidden_size and intermediate_size must be multiples of; gemv_grouped: the NAME of the mode's grouped expert GEMV (the ragged rows of a batch on
# a top-1 MoE layer: _expert_gemvs_top1).  A further mode is one entry here, its ops triple and its pair of public wrappers
# (generation.GenerationMixin); nothing else in this file or that one names a bit width.
DecodeMode = collections.namedtuple("DecodeMode", "bits words quantizer gemv multiple why gemv_grouped")
DECODE_MODES = {m.bits: m for m in (
    DecodeMode(8, "8-bit", "quantize_rows_w8", "gemv_w8", 16, "16 codes per 16-byte load", "gemv_grouped_w8"),            # row-wise absmax int8, bitsandbytes' weight format: (codes, scale), + half the decoder's bf16 bytes
    DecodeMode(4, "4-bit", "quantize_blocks_nf4", "gemv_w4", 64, "one absmax per block of 64 weights", "gemv_grouped_w4"),  # NF4: 4-bit codes, one fp32 absmax per 64 weights: (codes, absmax), + 0.28 of them
)}
DecodeWeights = collections.namedtuple("DecodeWeights", "mode copies epoch")    # LlamaStack.decode_weights while a mode is on


class LlamaStack:
    def __init__(self, cfg, device, init_std=0.02, seed=0):
        self.cfg, self.device = cfg, device
        d, ff, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size
        E = cfg.num_experts
        self.moe_layers = cfg.moe_layer_set()
        g = torch.Generator(device=device).manual_seed(seed)

        def rn(*shape, std=init_std, dtype=torch.bfloat16):
            return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * std).to(dtype)
        self.embed_tokens = rn(V, d)
        self.lm_head = rn(V, d)
        self.norm_w = torch.ones(d, dtype=torch.float32, device=device)
        self.layers = []
        for i in range(L):
            lw = {"qkv": rn(3 * d, d), "o": rn(d, d), "ln1": torch.ones(d, dtype=torch.float32, device=device),
                  "ln2": torch.ones(d, dtype=torch.float32, device=device)}
            if i in self.moe_layers:
                lw["wg"] = rn(E, d, dtype=torch.float32)
                lw["gu"] = rn(E, 2 * ff, d)
                lw["down"] = rn(E, d, ff)
                if cfg.use_residual:              # MoE.mlp (a dense copy of the expert) + MoE.coefficient = Linear(hidden, 2)
                    lw["res_gu"] = rn(2 * ff, d)
                    lw["res_down"] = rn(d, ff)
                    lw["coef_w"] = torch.zeros(8, d, dtype=torch.bfloat16, device=device)     # rows 2..7 are padding
                    lw["coef_w"][:2] = rn(2, d)
                    lw["coef_b"] = torch.zeros(8, dtype=torch.float32, device=device)
            else:
                lw["gu"] = rn(2 * ff, d)
                lw["down"] = rn(d, ff)
            self.layers.append(lw)
        self.cos, self.sin = _rope_tables(cfg.max_position_embeddings, cfg.head_dim, cfg.rope_theta, device)
        self.sin_neg = None                # -sin, for the LoRA backward's transposed RoPE (llama_lora.attach); grown with the tables
        self.training = True
        self.rts_uniform_provider = None   # callable(layer_idx, T, E) -> fp32 [T,E] gate draws (RTS uniforms / top-2 Gumbel) or None
        self.gate_pass = 0                 # forward passes so far: part of the key of the stateless gate-draw generator
        self.ep = None                     # ExpertParallel (expert_parallel.py) once enable_expert_parallel() sharded the experts
        self.lora = None                   # LoRAState: written by llama_lora.enable_lora / medplib.merge_and_unload, read by llama_lora and medplib
        # per-pass state (names and lifetimes are an interface: medplib.model_forward, bench.py, oracle/parity.py and the tests use them)
        self.needed_rows = None            # (rows int64, mask uint8) of the rows something reads: model_forward / a test sets and clears it around a pass; forward, forward_train read
        self.pruned_rows = None            # rows the last layer's MLP ran on: model_forward clears and reads it, _mlp_gather_scatter / forward_train write it
        self.layer_events = None           # a torch.cuda.Event per layer: model_forward creates them (gate_towers) for the towers, _mlp_gather_scatter records
        self.folded_layers = 0             # layers the last forward ran with folded norms: forward writes, bench.py / oracle/parity.py / tests read
        self.last_gate_inputs = None       # per MoE layer, the stream before the post-attention norm: forward(collect_routing=True) writes, oracle/parity.py reads
        self._draws_key = None             # what _draws_all was drawn for: _gate_draws writes and reads; generation._captured_steps and tests reset it to None
        self._draws_all = None             # fp32 [L * T * E] gate draws of one pass, all layers: _gate_draws writes and slices
        self.fuse_moe_gather_scatter = True   # top-1, one rank: dispatch / combine folded into the expert GEMMs
        self.fuse_decode_routing = True       # decode rows: post-attention norm + gate + routing in one launch
        self.group_expert_gemvs = GEMV_GROUPED   # ragged batch rows: one weight pass per expert (top-1: ops.gemv_grouped, or the quantised mode's grouped op; top-2: ops.gemv_grouped_top2_*), else the indexed / per-entry form
        self.decode_weights = None         # quantised decode mode: DecodeWeights(mode of DECODE_MODES, per layer {"qkv" | "o" | "gu" | "down": (codes, scales)}, ops.PARAM_EPOCH they were quantised at), or None (off): quantize_decode_weights / drop_decode_weights
        # RoPE in the qkv GEMM's epilogue (mp_gemm_qkv_rope_bf16) wants the q / k head rows interleaved in blocks of 32; the plain
        # fused qkv weight stays (decode GEMVs, the LoRA path's dgrad transposes, export), the interleaved copy (+3.2 GB of 288 at
        # 7B) serves every multi-row forward.  Rebuilt whenever the qkv weights change (refresh_fused_qkv).
        self.fuse_rope = cfg.head_dim == 128 and cfg.hidden_size % 256 == 0
        self.refresh_fused_qkv()

    def refresh_fused_qkv(self):
        """(Re)build the RoPE-interleaved copies of the fused qkv weights; call after anything that writes lw["qkv"]."""
        for lw in self.layers:
            if self.fuse_rope:
                lw["qkv_rope"] = ops.rope_interleave_qkv(lw["qkv"], self.cfg.num_attention_heads, self.cfg.head_dim)
            else:
                lw.pop("qkv_rope", None)
        self.refresh_folded_norms()

    def refresh_folded_norms(self):
        """config.fold_input_norm: the frozen weights with the norm weights multiplied into their columns — W' = bf16(W * ln_w[None, :]) — for the two
        consumer GEMMs of a top-1 MoE layer's RMSNorms (qkv + RoPE, experts' gate|up).  Call after anything that writes ln1 / ln2 / qkv / gu.
        (+ 0.46 GB per layer at 7B, E = 2: the unfolded weights stay for decode, export and the adapter path.)"""
        on = bool(getattr(self.cfg, "fold_input_norm", False)) and self.fuse_rope and self.cfg.top_k_experts == 1 and not self.cfg.use_residual
        for i, lw in enumerate(self.layers):
            lw.pop("qkv_rope_f", None); lw.pop("gu_f", None)
            if on and i in self.moe_layers:
                lw["qkv_rope_f"] = (lw["qkv_rope"].float() * lw["ln1"][None, :]).to(torch.bfloat16)
                lw["gu_f"] = (lw["gu"].float() * lw["ln2"][None, None, :]).to(torch.bfloat16)

    DECODE_WEIGHT_KEYS = ("qkv", "o", "gu", "down")

    def decode_weights_unsupported(self, bits):
        """Why this stack cannot decode from the copies of mode DECODE_MODES[bits] (a sentence), or None: one list for every mode."""
        cfg, mode = self.cfg, DECODE_MODES[bits]
        if any(i in self.moe_layers for i in range(len(self.layers))) and cfg.top_k_experts != 1:
            return f"top-2 expert routing has no {mode.words} expert GEMVs (top_k_experts == 1 only)"
        if cfg.use_residual:
            return "the residual MoE (use_residual) decodes through the GEMM path, which reads the bf16 weights"
        if self.ep is not None:
            return f"expert parallelism keeps the experts sharded; the {mode.words} expert GEMVs run on one rank"
        if self.lora is not None:
            return f"attached adapters rewrite the bf16 weights under the {mode.words} copies (adapters_merged()): call merge_and_unload() first"
        if cfg.hidden_size % mode.multiple or cfg.intermediate_size % mode.multiple:
            return f"hidden_size={cfg.hidden_size} and intermediate_size={cfg.intermediate_size} must be multiples of {mode.multiple} ({mode.why})"
        return None

    def quantize_decode_weights(self, bits):
        """Quantised decode mode DECODE_MODES[bits] on: copies (the mode's ops quantiser) of every layer's qkv, o, gate|up and down projections,
        dense [N, K] and expert [E, N, K] alike, beside the bf16 weights, which stay and serve prefill, training, export and the adapter merge.
        While self.decode_weights is set, every decode row (decode_step, forward with a KV cache at pos0 > 0) streams the copies.  lm_head,
        embed_tokens, the norms and the gate wg are not quantised.  Stamped with ops.PARAM_EPOCH: whoever decodes re-quantises when the
        parameters were written since.  NotImplementedError (and nothing changed, the other mode's copies included) where the mode is not built."""
        mode = DECODE_MODES[bits]
        why = self.decode_weights_unsupported(bits)
        if why is not None:
            raise NotImplementedError(f"{mode.words} decode weights: {why}")
        self.drop_decode_weights()         # whichever mode was on, before the new copies are allocated: one mode at a time, no higher memory peak
        quantize = getattr(ops, mode.quantizer)
        self.decode_weights = DecodeWeights(mode, [{k: quantize(lw[k]) for k in self.DECODE_WEIGHT_KEYS} for lw in self.layers], ops.PARAM_EPOCH)

    def drop_decode_weights(self):
        """Quantised decode mode off: the copies are dropped and every decode row reads the bf16 weights again."""
        self.decode_weights = None

    def _decode_copies(self, i):
        """Layer i's quantised copies of the mode that is on, or None: what a decode row hands down to _row_proj as copies."""
        return self.decode_weights.copies[i] if self.decode_weights is not None else None

    def _row_proj(self, lw, key, a, copies, **kw):
        """THE selector of a decode-row projection (at most 8 rows): the GEMV of the mode that is on, on the layer's quantised copies
        (_decode_copies(i), handed down only for a decode row), or the bf16 GEMV on lw[key]."""
        if copies is not None:
            return getattr(ops, self.decode_weights.mode.gemv)(a, *copies[key], **kw)
        return ops.gemv(a, lw[key], **kw)

    def enable_expert_parallel(self, ep):
        """Shard the experts over an expert-parallel group (DeepSpeed `ep_size`, medplib_moe_llama.py:604-614): every rank keeps the
        weights of its E/ep experts only; the gate `wg` stays replicated.  Call after the weights are loaded."""
        ids = ep.local_expert_ids()
        for i in self.moe_layers:
            lw = self.layers[i]
            for k in ("gu", "down", "gu_T", "down_T"):           # (+ the dgrad transposes when enable_lora() ran first)
                if k in lw:
                    lw[k] = lw[k][ids[0]:ids[-1] + 1].contiguous()
            for k in ("gu", "down"):                             # the expert-parallel training path keeps the unfused adapter kernels
                lw.pop(k + "_x", None)
                if self.lora is not None:
                    self.lora.ext.pop((i, k), None)
        self.ep = ep

    # ------------------------------------------------------------------ HF checkpoint layout
    def load_hf(self, sd, prefix=""):
        cfg = self.cfg
        d, ff = cfg.hidden_size, cfg.intermediate_size

        def put(dst, src):
            dst.copy_(src.to(device=dst.device, dtype=dst.dtype))
        put(self.embed_tokens, sd[prefix + "model.embed_tokens.weight"])
        put(self.lm_head, sd[prefix + "lm_head.weight"])
        put(self.norm_w, sd[prefix + "model.norm.weight"])
        for i, lw in enumerate(self.layers):
            p = f"{prefix}model.layers.{i}."
            for j, n in enumerate(("q", "k", "v")):
                put(lw["qkv"][j * d:(j + 1) * d], sd[p + f"self_attn.{n}_proj.weight"])
            put(lw["o"], sd[p + "self_attn.o_proj.weight"])
            put(lw["ln1"], sd[p + "input_layernorm.weight"])
            put(lw["ln2"], sd[p + "post_attention_layernorm.weight"])
            if i in self.moe_layers:
                put(lw["wg"], sd[p + "mlp.deepspeed_moe.gate.wg.weight"])
                for e in range(cfg.num_experts):
                    ep = p + f"mlp.deepspeed_moe.experts.deepspeed_experts.{e}."
                    put(lw["gu"][e], ops.swiglu_interleave(sd[ep + "gate_proj.weight"], sd[ep + "up_proj.weight"]))
                    put(lw["down"][e], sd[ep + "down_proj.weight"])
                if self.cfg.use_residual:
                    put(lw["res_gu"], ops.swiglu_interleave(sd[p + "mlp.mlp.gate_proj.weight"], sd[p + "mlp.mlp.up_proj.weight"]))
                    put(lw["res_down"], sd[p + "mlp.mlp.down_proj.weight"])
                    put(lw["coef_w"][:2], sd[p + "mlp.coefficient.weight"])
                    put(lw["coef_b"][:2], sd[p + "mlp.coefficient.bias"])
            else:
                put(lw["gu"], ops.swiglu_interleave(sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]))
                put(lw["down"], sd[p + "mlp.down_proj.weight"])
        self.refresh_fused_qkv()

    def export_hf(self, prefix=""):
        cfg = self.cfg
        d, ff = cfg.hidden_size, cfg.intermediate_size
        bf = torch.bfloat16
        sd = {prefix + "model.embed_tokens.weight": self.embed_tokens, prefix + "lm_head.weight": self.lm_head,
              prefix + "model.norm.weight": self.norm_w.to(bf)}
        for i, lw in enumerate(self.layers):
            p = f"{prefix}model.layers.{i}."
            for j, n in enumerate(("q", "k", "v")):
                sd[p + f"self_attn.{n}_proj.weight"] = lw["qkv"][j * d:(j + 1) * d]
            sd[p + "self_attn.o_proj.weight"] = lw["o"]
            sd[p + "input_layernorm.weight"] = lw["ln1"].to(bf)
            sd[p + "post_attention_layernorm.weight"] = lw["ln2"].to(bf)
            if i in self.moe_layers:
                sd[p + "mlp.deepspeed_moe.gate.wg.weight"] = lw["wg"]
                for e in range(cfg.num_experts):
                    ep = p + f"mlp.deepspeed_moe.experts.deepspeed_experts.{e}."
                    sd[ep + "gate_proj.weight"], sd[ep + "up_proj.weight"] = ops.swiglu_deinterleave(lw["gu"][e])
                    sd[ep + "down_proj.weight"] = lw["down"][e]
                if self.cfg.use_residual:
                    sd[p + "mlp.mlp.gate_proj.weight"], sd[p + "mlp.mlp.up_proj.weight"] = ops.swiglu_deinterleave(lw["res_gu"])
                    sd[p + "mlp.mlp.down_proj.weight"] = lw["res_down"]
                    sd[p + "mlp.coefficient.weight"] = lw["coef_w"][:2]
                    sd[p + "mlp.coefficient.bias"] = lw["coef_b"][:2].to(torch.bfloat16)
            else:
                sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = ops.swiglu_deinterleave(lw["gu"])
                sd[p + "mlp.down_proj.weight"] = lw["down"]
        return sd

    # ------------------------------------------------------------------ forward
    def capacity(self, T):
        """DeepSpeed _capacity: ceil(T / E * cf), at least min_capacity; top2gating passes 2 * cf."""
        cfg = self.cfg
        cf = cfg.capacity_factor if self.training else cfg.eval_capacity_factor
        return max(int(math.ceil(T / cfg.num_experts * cf * cfg.top_k_experts)), cfg.min_capacity)

    def _gate_draws(self, i, T, E, gumbel, pass_dev=None):
        """Random draws of the gate: an injected provider (tests: the same numbers go to the oracle) or, when the config asks for
        DeepSpeed's sampling behaviour, the stateless generator keyed by (seed, forward pass, layer).  pass_dev: decode_step's."""
        if self.rts_uniform_provider is not None:
            return self.rts_uniform_provider(i, T, E)
        if not self.cfg.moe_gate_sampling:
            return None
        # the generator is keyed by (seed, offset + index) and a pass's layers occupy consecutive offsets: ONE launch per forward pass draws
        # for all layers (the same numbers as a launch per layer, which sat between every layer's routing kernel and its expert GEMMs)
        L = len(self.layers)
        key = (self.gate_pass, T, E, bool(gumbel), pass_dev is not None)
        if self._draws_key != key:
            if pass_dev is not None:       # a decode step under a HIP graph: the pass number is read on the device (decode_step)
                self._draws_all = ops.gate_noise_dev(L * T * E, self.cfg.moe_gate_seed, pass_dev, L * T * E, gumbel, self.device)
            else:
                self._draws_all = ops.gate_noise(L * T * E, self.cfg.moe_gate_seed, self.gate_pass * L * T * E, gumbel, self.device)
            self._draws_key = key
        return self._draws_all[i * T * E:(i + 1) * T * E]

    def _expert_gemv_rows(self, T):
        """Whether T rows of a MoE layer take the per-row expert GEMVs (the decode rows): one rank, at most 8 rows, no residual MoE."""
        return self.ep is None and T <= 8 and not self.cfg.use_residual

    def _expert_gemvs_top1(self, lw, h, x, expert, slot, weight, copies=None, grouped=False):
        """Decode rows, top-1: each row streams its own expert's matrices (GEMV with a device-side expert index); the combine weight, the
        capacity drop and the residual ride in the down projection's epilogue.  Behind _mlp's routing and behind decode_step's fused one.
        grouped (the ragged rows of a batch): the rows that name the same expert share its weight pass — ops.gemv_grouped on the bf16 weights,
        the mode's own grouped op (DecodeMode.gemv_grouped) on its quantised copies; each has the bits of the indexed form it replaces;
        group_expert_gemvs = False keeps the indexed form (A/B), for every weight type."""
        if grouped and self.group_expert_gemvs:
            if copies is None:
                op, gu, down = ops.gemv_grouped, (lw["gu"],), (lw["down"],)
            else:
                op, gu, down = getattr(ops, self.decode_weights.mode.gemv_grouped), copies["gu"], copies["down"]
            act = op(h, *gu, expert, act=ops.ACT_SWIGLU_PAIR, row_keep=slot)
            return op(act, *down, expert, residual=x, row_scale=weight, row_keep=slot)
        if copies is not None:         # (the quantised gate|up GEMVs also skip a dropped row's weights; its act row stays unwritten and the down projection never reads it)
            act = self._row_proj(lw, "gu", h, copies, act=ops.ACT_SWIGLU_PAIR, w_index=expert, row_keep=slot)
        else:                      # (the bf16 kernel would skip it too, given row_keep; the recorded launch traces pin this call without it)
            act = self._row_proj(lw, "gu", h, copies, act=ops.ACT_SWIGLU_PAIR, w_index=expert)
        return self._row_proj(lw, "down", act, copies, residual=x, w_index=expert, row_scale=weight, row_keep=slot)

    def _expert_gemvs_top2(self, lw, h, x, expert, slot, weight, grouped=False):
        """Decode rows, top-2: the 2T (token, choice) entries stream their experts' matrices; the down projection adds both weighted expert
        outputs and the residual in moe_combine's order.  Behind _mlp's routing and behind decode_step's fused one.
        grouped (the ragged rows of a batch, two or more): the entries that name the same expert share its weight pass (ops.gemv_grouped_top2_gate_up /
        _down: at most min(E, 2T) expert MLPs read instead of 2T), with the bits of the per-entry pair; group_expert_gemvs = False keeps
        the per-entry pair (A/B)."""
        # A group of one keeps the per-entry pair: its two entries name two different experts, the same two weight streams either way, and the
        # grouped pair measured no faster there (103.8 against 104.9 us per layer, 5.180 against 5.193 ms per step with a spread of 0.025 in
        # the per-entry arm's own repeats: profiles/batch_decode.md).  The bits are the same either way.
        if grouped and self.group_expert_gemvs and h.shape[0] > 1:
            act = ops.gemv_grouped_top2_gate_up(h, lw["gu"], expert, slot)
            return ops.gemv_grouped_top2_down(act, lw["down"], expert, slot, weight, x)
        act = ops.gemv_top2_gate_up(h, lw["gu"], expert, slot)
        return ops.gemv_top2_down(act, lw["down"], expert, slot, weight, x)

    def _mlp(self, i, lw, h, x, gate=None, needed=None, rstd=None, pass_dev=None, copies=None, cap=None, seg=None):
        """x + MLP(h): h = post-attention RMSNorm output [T,d], x = residual stream [T,d]; gate = (logits, gates) when the caller's fused
        norm kernel already produced them (ops.rmsnorm_gate); needed = (rows, mask) when only those output rows are read (the last layer);
        rstd: the folded post-attention norm (h is None then); copies: the layer's quantised copies (_decode_copies) when the rows are decode rows; cap: the ragged rows of a batch (decode_step with `rows`) — that capacity (T: nothing dropped), no draws, the grouped expert GEMVs; seg = (seg_lens, seg_stride, capacities): the rows are the right-padded prompts of a batched prefill (forward with seg_lens) — every prompt routed as a pass of its own (ops.moe_route_top1_segments / _top2_segments), never the expert-GEMV rows.  Selects the branch -> (out, l_aux, (expert, slot, counts)); None, None when dense."""
        cfg, T = self.cfg, x.shape[0]
        if i not in self.moe_layers:
            if T <= 8:
                return self._row_proj(lw, "down", self._row_proj(lw, "gu", h, copies, act=ops.ACT_SWIGLU_PAIR), copies, residual=x), None, None
            act = ops.gemm(h, lw["gu"], act=ops.ACT_SWIGLU_PAIR)       # silu(gate)*up fused into the GEMM epilogue
            return ops.gemm(act, lw["down"], residual=x), None, None
        ragged = cap is not None
        E, k, cap = cfg.num_experts, cfg.top_k_experts, cap if ragged else self.capacity(T)
        logits, gates = gate if gate is not None else ops.moe_gate(h, lw["wg"])
        if seg is not None:        # (forward refused expert parallelism and the residual MoE: batch_rows_unsupported)
            if k == 1 and self.fuse_moe_gather_scatter:
                return self._mlp_gather_scatter(i, lw, h, x, gates, None, None, None, None, seg=seg)
            return self._mlp_dispatch_combine(i, lw, h, x, logits, gates, None, None, seg=seg)
        if k == 1 and self._expert_gemv_rows(T):
            # (no gate draws: random token selection only acts when an expert is over capacity; below cap >= T the draws are generated as usual)
            draws = None if cap >= T else self._gate_draws(i, T, E, False, pass_dev)
            expert, slot, weight, kept, counts, l_aux = ops.moe_route_top1(gates, cap, draws)
            return self._expert_gemvs_top1(lw, h, x, expert, slot, weight, copies, grouped=ragged), l_aux, (expert, slot, counts)
        if k == 2 and self._expert_gemv_rows(T):
            expert, slot, weight, kept, counts, l_aux = ops.moe_route_top2(gates, logits, cap, self._gate_draws(i, T, E, True, pass_dev))
            return self._expert_gemvs_top2(lw, h, x, expert, slot, weight, grouped=ragged), l_aux, (expert, slot, counts)
        if k == 1 and self.ep is None and self.fuse_moe_gather_scatter and not cfg.use_residual:
            return self._mlp_gather_scatter(i, lw, h, x, gates, cap, needed, rstd, pass_dev)
        return self._mlp_dispatch_combine(i, lw, h, x, logits, gates, cap, pass_dev)

    def _mlp_gather_scatter(self, i, lw, h, x, gates, cap, needed, rstd, pass_dev, seg=None):
        """Top-1 on one rank: the dispatch is a row gather in the gate|up GEMM's operand fetch and the combine (gate weight and the layer's
        residual add) a row scatter in the down GEMM's epilogue; every routed token's row is written exactly once.
        seg (_mlp): the segmented routing's slot_token / kept pair over slabs of sum(capacities) rows; a pad row is routed nowhere and keeps
        the residual stream, like a dropped token."""
        E, ff, T = self.cfg.num_experts, self.cfg.intermediate_size, x.shape[0]
        if seg is not None:
            cap = sum(seg[2])
            expert, slot, weight, kept, counts, l_aux, slot_token = ops.moe_route_top1_segments(gates, *seg, want_slot_token=True)
        else:
            expert, slot, weight, kept, counts, l_aux, slot_token = ops.moe_route_top1(gates, cap, self._gate_draws(i, T, E, False, pass_dev), want_slot_token=True)
        act = torch.empty((E, cap, ff), dtype=torch.bfloat16, device=x.device)
        if needed is not None:
            self.pruned_rows = int(needed[0].numel())      # the pruning HAPPENED (model_forward reports only this)
            # the last layer: only the rows something reads go through the experts (the routing above saw every token: capacity drops,
            # l_aux and the counts are those of the whole batch); a row that is not computed keeps the residual stream, which nobody reads
            slot_token, kept = ops.moe_filter_slots(slot_token, kept, needed[1])
        if ops.GEMM_TIMER is not None:
            ops.GEMM_TIMER.batched_tag = i          # the expert GEMMs are credited with the rows `kept` holds after the region
        if self.layer_events is not None and i < len(self.layer_events):
            self.layer_events[i].record()   # "layer i's expert GEMMs start here": what the frozen towers of the NEXT step gate their layers on (medplib.model_forward)
        if rstd is not None:        # folded post-attention norm: the experts read the raw stream, W carries ln2, the epilogue applies rstd
            ops.gemm_batched_rows(x, lw["gu_f"], act, kept, a_rows=slot_token, act=ops.ACT_SWIGLU_PAIR, rows_stride=cap, a_row_scale=rstd)
        else:
            ops.gemm_batched_rows(h, lw["gu"], act, kept, a_rows=slot_token, act=ops.ACT_SWIGLU_PAIR, rows_stride=cap)
        # The combine writes INTO the residual stream (out = residual = x).  Every (routed row, 16-byte column piece) has exactly one owner in
        # the down projection's epilogue — a tile, or one unit's share of a split tail tile — which reads the residual piece and stores the sum
        # at the same address; a capacity-dropped token's row is left as it is, which is DeepSpeed's result for it (x + 0) (same bits as the
        # unfused form: test_moe_fused_gather_scatter_matches_unfused).  No gradient flows here (the LoRA path keeps its own forward).
        ops.gemm_batched_rows(act, lw["down"], x, kept, c_rows=slot_token, c_scale=weight, residual=x, rows_stride=cap)
        return x, l_aux, (expert, slot, counts)

    def _mlp_dispatch_combine(self, i, lw, h, x, logits, gates, cap, pass_dev, seg=None):
        """The generic MoE branch (top-2, unfused top-1, expert parallelism, residual MoE): dispatch into capacity slabs, batched expert GEMM pair, combine.
        seg (_mlp): the segmented routing's entry arrays over slabs of sum(capacities) rows; a pad row's entries are dropped ones."""
        cfg = self.cfg
        E, ff, d, k, T = cfg.num_experts, cfg.intermediate_size, cfg.hidden_size, cfg.top_k_experts, x.shape[0]
        if seg is not None:
            cap = sum(seg[2])
            if k == 1:
                expert, slot, weight, kept, counts, l_aux = ops.moe_route_top1_segments(gates, *seg)
            else:
                expert, slot, weight, kept, counts, l_aux = ops.moe_route_top2_segments(gates, logits, *seg)
        elif k == 1:
            expert, slot, weight, kept, counts, l_aux = ops.moe_route_top1(gates, cap, self._gate_draws(i, T, E, False, pass_dev))
        else:
            expert, slot, weight, kept, counts, l_aux = ops.moe_route_top2(gates, logits, cap, self._gate_draws(i, T, E, True, pass_dev))
        if self.ep is not None:
            # slabs of capx + 1 rows: capx = the capacity agreed over the expert-parallel group for this pass (ranks see different
            # T), the extra row is the header that carries the row count through the same all-to-all (expert_parallel.py)
            capx = self.ep.exchange_capacity(cap, key=self.gate_pass)
            buf = ops.moe_dispatch(h, expert, slot, E, capx + 1, top_k=k)
            y = self._experts_parallel(lw, buf, kept, capx)
            if cfg.use_residual:
                raise NotImplementedError("residual MoE with ep_size > 1")
            return ops.moe_combine(y, expert, slot, weight, x, capx, top_k=k), l_aux, (expert, slot, counts)
        buf = ops.moe_dispatch(h, expert, slot, E, cap, top_k=k)
        act = torch.empty((E, cap, ff), dtype=torch.bfloat16, device=h.device)
        if ops.GEMM_TIMER is not None:
            ops.GEMM_TIMER.batched_tag = i              # (credited with the kept rows: every token visits k experts unless dropped)
        ops.gemm_batched(buf, lw["gu"], act, m_dev=kept, act=ops.ACT_SWIGLU_PAIR)
        y = torch.empty((E, cap, d), dtype=torch.bfloat16, device=h.device)
        ops.gemm_batched(act, lw["down"], y, m_dev=kept)
        if cfg.use_residual:
            return self._residual_mix(lw, h, x, ops.moe_combine(y, expert, slot, weight, None, cap, top_k=k)), l_aux, (expert, slot, counts)
        return ops.moe_combine(y, expert, slot, weight, x, cap, top_k=k), l_aux, (expert, slot, counts)

    def _residual_mix(self, lw, h, x, moe):
        """Residual MoE: the routed output and a dense MLP of the same input, mixed by a learned two-way softmax."""
        mlp = ops.gemm(ops.gemm(h, lw["res_gu"], act=ops.ACT_SWIGLU_PAIR), lw["res_down"])
        coef = ops.gemm(h, lw["coef_w"], bias=lw["coef_b"])
        return ops.moe_residual_mix(x, moe, mlp, coef)

    def _experts_parallel(self, lw, buf, kept, cap):
        """MOELayer with ep_size > 1: all-to-all the routed rows to the ranks that own the experts, run each local expert over the
        [ep] capacity slabs it received (one batched GEMM pair per local expert, the slab row counts travel with the rows), and
        all-to-all the outputs back (sharded_moe.py MOELayer.forward; collectives C3 of SURVEY §2.5)."""
        cfg, ep = self.cfg, self.ep
        ff, d = cfg.intermediate_size, cfg.hidden_size
        recv, counts = ep.dispatch(buf, kept)                      # [ep, E_local, cap + 1, d] (row cap = header), [ep, E_local]
        counts_t = counts.t().contiguous()                         # [E_local, ep]: per local expert, rows from each source rank
        y = torch.empty((ep.ep, ep.E_local, cap, d), dtype=recv.dtype, device=recv.device)
        for e in range(ep.E_local):
            a = recv[:, e, :cap]                                   # [ep, cap, d] view, batch stride E_local*(cap+1)*d
            act = torch.empty((ep.ep, cap, ff), dtype=torch.bfloat16, device=buf.device)
            ops.gemm_batched(a, lw["gu"][e].unsqueeze(0).expand(ep.ep, -1, -1), act, m_dev=counts_t[e], act=ops.ACT_SWIGLU_PAIR)
            ops.gemm_batched(act, lw["down"][e].unsqueeze(0).expand(ep.ep, -1, -1), y[:, e], m_dev=counts_t[e])
        return ep.combine(y)

    def ensure_positions(self, n):
        """Grow cos / sin (and sin_neg) to cover positions 0 .. n - 1, as HF 4.31's LlamaRotaryEmbedding regrows its cache past
        max_position_embeddings.  Only the new rows are computed (same fp32 formula), the existing ones are kept as they are, so
        every row already in use stays bit-identical.  Growth replaces the tensors: a captured graph holding the old pointers
        would read freed memory, so callers grow before capturing (new_kv_cache)."""
        rows = rope_rows_for(int(n), self.cos.shape[0])
        if rows == self.cos.shape[0]:
            return
        cfg = self.cfg
        cos_new, sin_new = _rope_tables(rows, cfg.head_dim, cfg.rope_theta, self.device, start=self.cos.shape[0])
        self.cos = torch.cat([self.cos, cos_new]).contiguous()
        self.sin = torch.cat([self.sin, sin_new]).contiguous()
        if self.sin_neg is not None:
            self.sin_neg = (-self.sin).contiguous()

    def new_kv_cache(self, batch, max_len):
        """KV cache for `evaluate()`'s greedy decode (HF `use_cache=True`, MedPLIB.py:592-606): post-RoPE K and V per layer, and "err", the
        int32 word the bounded decode kernels set (MP_POS_ERR_*) when a step's position has no table or cache row.  The RoPE tables are
        grown to max_len HERE, before generation._captured_steps captures their pointers (growing after the capture would leave the graph reading the
        freed tables)."""
        cfg = self.cfg
        self.ensure_positions(max_len)
        shape = (batch, max_len, cfg.num_attention_heads, cfg.head_dim)
        return {"len": 0, "k": [torch.empty(shape, dtype=torch.bfloat16, device=self.device) for _ in self.layers],
                "v": [torch.empty(shape, dtype=torch.bfloat16, device=self.device) for _ in self.layers],
                "err": torch.zeros(1, dtype=torch.int32, device=self.device)}

    def _lin(self, lw, key, a, copies=None, **kw):
        """The projection lw[key] of a [T, K]: a handful of rows (the single-token decode steps) are a weight stream -> GEMV kernel (HBM-bound,
        _row_proj), else GEMM."""
        return self._row_proj(lw, key, a, copies, **kw) if a.shape[0] <= 8 else ops.gemm(a, lw[key], **kw)

    def _qkv(self, lw, x, S, pos0, folded, copies=None):
        """input_layernorm + fused qkv projection + RoPE of the rows x [B*S, d] at positions pos0 .. pos0 + S - 1 -> qkv [B*S, 3d]."""
        cfg = self.cfg
        H, D, (T, d) = cfg.num_attention_heads, cfg.head_dim, x.shape
        if folded:                         # x -> rstd1; qkv = (x W'^T) * rstd1 -> RoPE
            rstd1, _, _ = ops.rmsnorm_gate_rstd(x, lw["ln1"], cfg.rms_norm_eps)
            return ops.gemm_qkv_rope(x, lw["qkv_rope_f"], self.cos, self.sin, S, H, D, pos_offset=pos0, out=ops.padded_rows(T, 3 * d, x.device), row_scale=rstd1)
        h = ops.rmsnorm(x, lw["ln1"], cfg.rms_norm_eps)
        if self.fuse_rope and T > 8:       # RoPE in the epilogue (row stride of the qkv buffer kept off multiples of 8 KiB: ops.padded_rows)
            return ops.gemm_qkv_rope(h, lw["qkv_rope"], self.cos, self.sin, S, H, D, pos_offset=pos0, out=ops.padded_rows(T, 3 * d, x.device))
        qkv = self._lin(lw, "qkv", h, copies)
        ops.rope_qk_(qkv, self.cos, self.sin, S, H, D, pos_offset=pos0)
        return qkv

    def _post_attention_norm(self, i, lw, x, folded):
        """post_attention_layernorm of the stream x -> (h, gate, rstd) as _mlp takes them.  Folded: rstd2 and the gate (from HF's bf16 h), no h (the
        experts read x with W''); MoE layer of an rmsnorm_gate dimension: norm and gate in one pass over the rows (the two kernels' bits); else the norm."""
        cfg = self.cfg
        if folded:
            rstd2, lg, gt = ops.rmsnorm_gate_rstd(x, lw["ln2"], cfg.rms_norm_eps, lw["wg"])
            return None, (lg, gt), rstd2
        if i in self.moe_layers and x.shape[1] in ops.RMSNORM_GATE_DIMS and x.shape[0] > 8:
            h, lg, gt = ops.rmsnorm_gate(x, lw["ln2"], cfg.rms_norm_eps, lw["wg"])
            return h, (lg, gt), None
        return ops.rmsnorm(x, lw["ln2"], cfg.rms_norm_eps), None, None

    def forward(self, inputs_embeds, key_valid=None, collect_routing=False, kv_cache=None, seg_lens=None):
        """inputs_embeds [B,S,d] bf16; key_valid uint8 [B,S] (1 = real token) or None.
        With kv_cache: the S new tokens sit at positions cache.len .. cache.len+S-1, their K/V are appended and attention runs
        over the whole cache (prefill when cache.len == 0, single-token decode afterwards).
        seg_lens (a list of B ints): the batched prefill of a decode group — row b is a prompt of seg_lens[b] positions, right-padded to S,
        into an EMPTY kv_cache and without key_valid (right padding under the causal mask: no real query sees a pad key).  Everything but the
        routing is the [B, S] pass; a MoE layer routes every prompt as a pass of its own, at capacity(seg_lens[b]) (ops.moe_route_top1_segments /
        _top2_segments: no prompt loses an expert slot to a batch-mate or to padding), through the expert GEMMs whatever B * S is (never the
        expert GEMVs of the decode rows, never the folded norms); the pad rows are routed nowhere and only carry the residual stream, and
        what they leave in the hidden states and in the cache is for the caller to ignore.  One pass: gate_pass advances by one.
        ValueError for a cache that is missing or not empty, key_valid, or a length outside 1..S; NotImplementedError where
        batch_rows_unsupported() says so — both before any state changes.
        Returns (last_hidden_state after the final RMSNorm [B,S,d], [l_aux per MoE layer], routing or None)."""
        cfg = self.cfg
        B, S, d = inputs_embeds.shape
        H, D = cfg.num_attention_heads, cfg.head_dim
        seg = None
        if seg_lens is not None:
            seg_lens = [int(n) for n in seg_lens]
            if kv_cache is None or kv_cache["len"] != 0 or key_valid is not None:
                raise ValueError("LlamaStack.forward: seg_lens is the batched prefill of a decode group: it needs an empty kv_cache and no key_valid")
            if len(seg_lens) != B or not all(1 <= n <= S for n in seg_lens):
                raise ValueError(f"LlamaStack.forward: seg_lens={seg_lens} must hold {B} lengths in 1..{S}")
            why = self.batch_rows_unsupported()
            if why is not None:
                raise NotImplementedError(f"forward with seg_lens: {why}")
            seg = (seg_lens, S, [self.capacity(n) for n in seg_lens])
        x = inputs_embeds.reshape(B * S, d)
        aux, routing, gate_inputs = [], [], []
        nr = self.needed_rows               # (rows, mask) from model_forward: the output rows something reads, or None
        needed = nr if (nr is not None and not collect_routing and kv_cache is None and nr[1].numel() == B * S) else None
        self.gate_pass += 1
        pos0 = kv_cache["len"] if kv_cache is not None else 0
        if kv_cache is not None and pos0 + S > kv_cache["k"][0].shape[1]:
            raise ValueError(f"LlamaStack.forward: positions {pos0}..{pos0 + S - 1} do not fit the KV cache of {kv_cache['k'][0].shape[1]} rows")
        self.ensure_positions(pos0 + S)
        # folded norms (config.fold_input_norm): frozen top-1 MoE layers of 320-row-kernel shapes, one rank, no KV cache
        fold = ("qkv_rope_f" in self.layers[0] if self.layers else False) and kv_cache is None and self.ep is None and self.fuse_moe_gather_scatter \
            and d in ops.RMSNORM_GATE_DIMS and ops.gemm_fold_ok(B * S, 3 * d, d) and ops.gemm_fold_ok(self.capacity(B * S), 2 * cfg.intermediate_size, d)
        self.folded_layers = 0
        last = len(self.layers) - 1
        # quantised decode mode: only a decode row (a cached step behind the prefill) streams the copies, never a short prefill or a cache-free pass
        quant_row = self.decode_weights is not None and kv_cache is not None and pos0 > 0 and B * S <= 8
        for i, lw in enumerate(self.layers):
            folded = fold and "qkv_rope_f" in lw
            copies = self._decode_copies(i) if quant_row else None
            q5 = self._qkv(lw, x, S, pos0, folded, copies).unflatten(0, (B, S)).unflatten(2, (3, H, D))
            if kv_cache is not None:
                kv_cache["k"][i][:, pos0:pos0 + S].copy_(q5[:, :, 1])
                kv_cache["v"][i][:, pos0:pos0 + S].copy_(q5[:, :, 2])
            if kv_cache is not None and pos0 > 0:
                assert S == 1 and key_valid is None, "cached decode is single-token, un-padded (the reference evaluates with batch 1)"
                attn = ops.attention(q5[:, :, 0], kv_cache["k"][i][:, :pos0 + 1], kv_cache["v"][i][:, :pos0 + 1], causal=False)
            else:
                attn = ops.attention(q5[:, :, 0], q5[:, :, 1], q5[:, :, 2], causal=True, key_valid=key_valid)
            x = self._lin(lw, "o", attn.view(B * S, d), copies, residual=x)
            # (tests / parity only: the layer's own gate input, copied before the combine writes the MLP output into the residual stream — the
            #  layer-local routing check of oracle/parity.py recomputes the gate from it)
            x_gate_in = x.clone() if (collect_routing and i in self.moe_layers) else None
            h, gate, rstd = self._post_attention_norm(i, lw, x, folded)
            # (the last layer's row set goes to _mlp whatever produced the gate: only the top-1 gather / scatter branch prunes, a dense layer ignores it)
            x, l_aux, r = self._mlp(i, lw, h, x, gate=gate, needed=needed if i == last else None, rstd=rstd, copies=copies, seg=seg)
            if l_aux is not None:
                aux.append(l_aux)
                if collect_routing:
                    routing.append(r)
                    gate_inputs.append(x_gate_in)
            self.folded_layers += int(folded)
        if kv_cache is not None:
            kv_cache["len"] = pos0 + S
        out = ops.rmsnorm(x, self.norm_w, cfg.rms_norm_eps)
        if collect_routing:
            self.last_gate_inputs = gate_inputs            # per MoE layer: the residual stream in front of the post-attention norm (oracle/parity.py)
        return out.view(B, S, d), aux, (routing if collect_routing else None)

    def batch_rows_unsupported(self):
        """Why this stack cannot decode ragged batch rows (decode_step with `rows`; generate_batch), a sentence, or None.  A row of a batch is
        routed as generate() routes it (T = 1: nothing dropped, no draws), so what needs the other rows or a draw is refused."""
        cfg = self.cfg
        if cfg.moe_gate_sampling or self.rts_uniform_provider is not None:
            return "the gate's random draws (moe_gate_sampling / an injected draw provider) are keyed on the rows of one pass"
        if cfg.use_residual:
            return "the residual MoE (use_residual) decodes through the GEMM path, which drops rows by the batch's capacity"
        if self.ep is not None:
            return "expert parallelism routes through the capacity slabs of the expert-parallel group"
        return None

    def decode_step(self, emb, kv_cache, counters, pass_dev=None, rows=None):
        """One token per sequence against the KV cache with the cache length held ON THE DEVICE (`counters` int32 [2] =
        [position of the new token, number of valid keys after appending it]): no launch argument depends on the step, so the
        whole step can be captured once into a HIP graph and replayed per token (evaluate()).  emb [B, 1, d] -> hidden [B, 1, d].
        The caller advances `counters` (ops.advance_ints) after the step.
        rows = (position int32 [B], keys int32 [B]) in place of `counters` (None then): every sequence has its OWN length — the ragged prompts
        of generate_batch as the rows of one step.  The layer body then takes the unfused qkv branch (the norm-folded launches have no per-row
        twin), ops.decode_rope_append_rows and ops.attention_decode_rows, and routes a MoE layer's rows with a capacity of B and no draws (no
        row is dropped because of its batch-mates: a row's answer does not depend on the others); a top-1 layer's rows share one weight pass
        per expert (ops.gemv_grouped; under a quantised mode its own grouped op on the copies: ops.gemv_grouped_w8 / _w4), and so do a top-2
        layer's 2B (row, choice) entries on the bf16 weights (ops.gemv_grouped_top2_gate_up / _down; B = 1 keeps the per-entry pair, which
        streams the same two experts).  NotImplementedError
        before any state changes where batch_rows_unsupported() says so.
        Reproducibility note (round-4 advisor): the narrow projections (o_proj, down) take the K-split GEMV when B == 1 or an expert index is
        given and the shared-weight form otherwise; the two add their partial dot products in different orders, so the SAME prompt decoded at
        batch 1 and at batch 2 may differ in the last fp32 bit of those projections (and, at a near-tie of two logits, in a greedy token).
        Within one batch size every step is bit-reproducible; MP_GEMV_KSPLIT=0 selects the shared form for every batch size.
        pass_dev (int32 [1] on the device, or None): the number of this forward pass, read on the device by the gate's random draws
        (moe_gate_sampling) instead of the host counter `gate_pass` — a captured step then draws, at every replay, what the token-by-token
        loop draws for that pass; the caller advances it with the counters."""
        cfg = self.cfg
        ragged = rows is not None
        if ragged:
            why = self.batch_rows_unsupported()
            if why is not None:
                raise NotImplementedError(f"decode_step with per-row lengths: {why}")
            pos_rows, key_rows = rows
        B, _, d = emb.shape
        H, D, E, k = cfg.num_attention_heads, cfg.head_dim, cfg.num_experts, cfg.top_k_experts
        x = emb.reshape(B, d)
        self.gate_pass += 1
        # input_layernorm inside the qkv GEMV (same bits, one launch less per layer); the norm-folded launches have no quantised twins and no
        # per-row twin: those modes take the unfused branches
        fold = not ragged and self.decode_weights is None and ops.gemv_rmsnorm_ok(B, d, head_dim=D, swiglu_n=2 * cfg.intermediate_size)
        for i, lw in enumerate(self.layers):
            copies = self._decode_copies(i)
            if fold:                                            # norm + projection + RoPE + cache append: one launch, the three launches' bits
                qkv = ops.gemv_rmsnorm_rope_append(x, lw["ln1"], cfg.rms_norm_eps, lw["qkv"], self.cos, self.sin, kv_cache["k"][i],
                                                   kv_cache["v"][i], counters[0:1], H, D, err=kv_cache["err"])
            else:
                qkv = self._row_proj(lw, "qkv", ops.rmsnorm(x, lw["ln1"], cfg.rms_norm_eps), copies)
                if ragged:
                    ops.decode_rope_append_rows(qkv, self.cos, self.sin, kv_cache["k"][i], kv_cache["v"][i], pos_rows, H, D, err=kv_cache["err"])
                else:
                    ops.decode_rope_append(qkv, self.cos, self.sin, kv_cache["k"][i], kv_cache["v"][i], counters[0:1], H, D, err=kv_cache["err"])
            q4 = qkv.view(B, 1, 3, H, D)[:, :, 0]
            if ragged:
                attn = ops.attention_decode_rows(q4, kv_cache["k"][i], kv_cache["v"][i], key_rows)
            else:
                attn = ops.attention(q4, kv_cache["k"][i], kv_cache["v"][i], causal=False, sk_dev=counters[1:2])
            x = self._row_proj(lw, "o", attn.view(B, d), copies, residual=x)
            # post-attention norm + gate + routing in ONE launch, then the expert GEMVs of _mlp's decode-row branches (the separate kernels' bits)
            if i in self.moe_layers and self.fuse_decode_routing and self._expert_gemv_rows(B) and k in (1, 2):
                cap = B if ragged else self.capacity(B)         # (ragged rows: generate()'s routing of each row, where nothing can be dropped)
                if k == 1:
                    draws = None if cap >= B else self._gate_draws(i, B, E, False, pass_dev)
                    h, expert, slot, weight, _, _, _ = ops.decode_norm_gate_route(x, lw["ln2"], cfg.rms_norm_eps, lw["wg"], cap, draws)
                    x = self._expert_gemvs_top1(lw, h, x, expert, slot, weight, copies, grouped=ragged)
                else:
                    draws = self._gate_draws(i, B, E, True, pass_dev)
                    h, expert, slot, weight, _, _, _ = ops.decode_norm_gate_route_top2(x, lw["ln2"], cfg.rms_norm_eps, lw["wg"], cap, draws)
                    x = self._expert_gemvs_top2(lw, h, x, expert, slot, weight, grouped=ragged)
            elif fold and i not in self.moe_layers:
                # dense layer: post_attention_layernorm inside the gate|up GEMV (same bits as rmsnorm + gemv), then the down projection
                act = ops.gemv_rmsnorm(x, lw["ln2"], cfg.rms_norm_eps, lw["gu"], act=ops.ACT_SWIGLU_PAIR)
                x = ops.gemv(act, lw["down"], residual=x)
            else:
                x, _, _ = self._mlp(i, lw, ops.rmsnorm(x, lw["ln2"], cfg.rms_norm_eps), x, pass_dev=pass_dev, copies=copies, cap=B if ragged else None)
        return ops.rmsnorm(x, self.norm_w, cfg.rms_norm_eps).view(B, 1, d)

    def next_token_logits(self, hidden_row):
        """fp32 logits of one position: lm_head(hidden).float() (medplib_moe_llama.py:388-389).  hidden_row [n, d] bf16."""
        h = hidden_row.contiguous()
        if h.shape[0] <= 8:
            return ops.gemv(h, self.lm_head, out_dtype=torch.float32)
        return ops.gemm(h, self.lm_head, out_dtype=torch.float32)

    def cross_entropy(self, last_hidden, sup_rows, sup_labels, aux):
        """CE over supervised rows only (row-wise op; unsupervised rows never reach the loss — SURVEY B.8):
        fp32 logits = lm_head(hidden[sup_rows]) (medplib_moe_llama.py:388-389), mean CE (:392-408),
        + router_aux_loss_coef * sum(l_aux) (:410-421).  sup_rows int64 [n] flat row ids, sup_labels int64 [n]."""
        cfg = self.cfg
        d = cfg.hidden_size
        if sup_rows.numel() == 0:
            return torch.full((1,), float("nan"), dtype=torch.float32, device=last_hidden.device)
        rows = ops.gather_rows_bf16_to_f32(last_hidden.view(-1, d), sup_rows)
        rows = ops.cast_to_bf16(rows)                     # exact: the rows were bf16
        logits = ops.gemm(rows, self.lm_head, out_dtype=torch.float32)
        row_loss = ops.cross_entropy_rows(logits, sup_labels)
        add = torch.cat(aux) if (aux and cfg.router_aux_loss_coef != 0.0) else None
        return ops.mean_plus(row_loss, 1.0, add, cfg.router_aux_loss_coef)
