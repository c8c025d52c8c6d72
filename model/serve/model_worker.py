"""Surface walk of the serving worker — what the reference's `model/serve/model_worker.py` does with the model for one request, written for
this build (no statement of the reference script is carried).

The reference worker, in order, and where this module does the same: `load_pretrained_model(model_path, ..., device_map=, vision_pretrained=)`
(:99-100; here `open_model`) -> per request `generate_stream(params)` (:231-541): the image from base64, ResizeLongestSide + pad for SAM
(256) and for CLIP (336) (:248-265), region masks resized like the CLIP image and taken at every 14th pixel (:272-279), temperature / top_p /
max_new_tokens (capped at 1024) / stop read from the request (:287-300), the prompt tokenised with the `<image>` placeholder and one region
placeholder between every `<region>` `</region>` pair (:302-313), the source cut to context_len - max_new_tokens - 8 tokens (:317-318), then
its own token loop: argmax below temperature 1e-4, else softmax(logits / temperature) + multinomial (:420-425), a message every
--stream-interval tokens, at the last token and at a stop (:441), the text cut at the last occurrence of the stop string (:442-446), and after
a stop the mask of the first <SEG> as the sparse [row, col] list of sigmoid > 0.1 (:449-529).  Messages are
`json.dumps({"text", "mask", "height", "width", "error_code": 0}).encode() + b"\\0"` (:531-538).  Here the token loop is
`MedPLIBForCausalLM.generate_stream`: the draw and the pick run on the device inside the captured decode step, top_p is read and ignored as in
the reference, and every request takes its sampling seed from torch's global generator, where the reference's multinomial takes its draws
(torch.manual_seed makes a sequence of requests repeatable).  With --apply-top-p the request's top_p (the front end's slider) and an
optional top_k (default 0: none) truncate the distribution before the draw — HF's top-k, then top-p, in the same captured step
(ops.sample_rows_filtered); without the flag a request is served exactly as the reference serves it.

Several requests at once: `ModelWorker.generate_stream_gate_batch(params_list)` serves the requests a server holds in list order in groups
of min(8, --limit-model-concurrency) — the requests of a group are the rows of ONE decode step (`MedPLIBForCausalLM.generate_stream_batch`:
one pass over the weights per token for the group, every row drawn and picked at its own temperature, top_p / top_k, seed, max_new_tokens
and stop) — and yields (index in params_list, message bytes), every message in generate_stream's format.  Both loops parse a request with
one helper (`_request`) and build a message with one (`_message`); seeds are drawn from torch's global generator in list order.  Where the
model refuses batch rows — moe_gate_sampling (the gate's draws are keyed on the rows of one pass), the residual MoE, expert parallelism —
the batch loop falls back to one request at a time through `generate_stream`, in the same (index, message) shape.  The shipped 7B config
has moe_gate_sampling ON: such a model is served one by one until it is switched off.

Out of scope: the HTTP server (FastAPI / uvicorn), the controller registration, the heartbeat thread and the concurrency semaphore;
--limit-model-concurrency is parsed and sizes the groups of `generate_stream_gate_batch` for a server built around it or around
`ModelWorker.generate_stream_gate`.

`images` / `region_masks` of a request: base64 strings as the reference's clients send them (decoded with Pillow, which is imported only then)
or uint8 arrays ([H, W, 3] RGB, [H, W]).  --load-8bit (reference :72,100,642 -> builder.py:39, bitsandbytes) is a SPEED mode here, not a memory mode:
`MedPLIBForCausalLM.enable_decode_8bit` adds int8 copies of the decoder projections in bitsandbytes' row-wise absmax format and every decode
step streams them (half the bytes per token); the bf16 weights stay for the prefill, the activations stay bf16 and lm_head is not quantised.
--load-4bit, --load-fp16 and any --precision but bf16 stay refused.  `FLAG_TABLE` holds the reference's command line as data; additions of this build: --precision, --apply-top-p."""
import argparse
import base64
import io
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = str(Path(__file__).resolve().parents[2])
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from medplib_amd import preprocess as P                                                             # noqa: E402
from medplib_amd.dataset import tokenize_with_image_tokens                                          # noqa: E402
from utils.utils import DEFAULT_IMAGE_TOKEN                                                         # noqa: E402

OFF = "off-by-default switch"
FLAG_TABLE = (
    # reference CLI, model/serve/model_worker.py:605-628: (name, default, kind)
    ("host", "localhost", str), ("port", 21002, int), ("worker-address", "http://localhost:21002", str),
    ("controller-address", "http://localhost:21001", str), ("model-path", "facebook/opt-350m", str), ("model-base", None, str),
    ("model-name", "medplib", str), ("vision_pretrained", "../huggingface_models/sam-med2d_b.pth", str), ("multi-modal", False, OFF),
    ("keep-aspect-ratio", False, OFF), ("num-gpus", 1, int), ("limit-model-concurrency", 5, int), ("stream-interval", 1, int),
    ("no-register", False, OFF), ("load-8bit", False, OFF), ("load-4bit", False, OFF), ("load-fp16", False, OFF),
    ("add_region_feature", False, OFF), ("image_w", 336, int), ("image_h", 336, int), ("device_map", "cpu", str),
    # ---- this build's addition
    ("precision", "bf16", ("fp32", "bf16", "fp16", "int8", "int4")),
    ("apply-top-p", False, OFF),         # honour the request's top_p (and an optional top_k); the reference reads top_p and drops it
)
MAX_NEW_TOKENS_CAP = 1024
MASK_THRESHOLD = 0.1


def parse_args(argv):
    ap = argparse.ArgumentParser(description="MedPLIB serving worker: surface walk of the reference worker")
    for name, default, kind in FLAG_TABLE:
        if kind == OFF:
            ap.add_argument("--" + name, action="store_true", default=default)
        elif isinstance(kind, tuple):
            ap.add_argument("--" + name, default=default, type=str, choices=list(kind))
        else:
            ap.add_argument("--" + name, default=default, type=kind)
    return ap.parse_args(argv)


def check_placement(args):
    """This build computes in bf16 on the GPU: every other --precision / --device_map (the reference's default is 'cpu') and the 4-bit /
    fp16 loads are refused, like --cpu_only in the eval walk.  --load-8bit passes: the decode steps then stream 8-bit weight copies
    (ModelWorker.__init__).  --load-4bit stays refused by the worker; the model has the mode (MedPLIBForCausalLM.enable_decode_4bit())."""
    if args.device_map != "cuda":
        raise NotImplementedError(f"--device_map {args.device_map}: this build has no CPU path (the HIP library is the only implementation); "
                                  "pass --device_map cuda")
    if args.precision != "bf16" or args.load_4bit or args.load_fp16:
        raise ValueError("this build computes in bf16 (the worker's own precision): --precision bf16, no --load-4bit / --load-fp16 "
                         "(--load-8bit: 8-bit weight copies for the decode steps, activations in bf16; NF4 copies: the model's "
                         "enable_decode_4bit(), not a worker flag)")


def open_model(args, tokenizer=None):
    """Construction half of the walk (load_pretrained_model): -> the model on the GPU, frozen, in eval mode."""
    check_placement(args)
    from model.MedPLIB import MedPLIBForCausalLM
    model = MedPLIBForCausalLM.from_pretrained(args.model_path, torch_dtype=torch.bfloat16, low_cpu_mem_usage=True,
                                               vision_pretrained=args.vision_pretrained, test_only=True)
    if tokenizer is not None:
        model.resize_token_embeddings(len(tokenizer))
    model.to(dtype=torch.bfloat16, device=0)
    for _, p in model.named_parameters():
        p.requires_grad = False
    return model.eval()


def _as_array(item, mode):
    """A request's image or region mask -> uint8 array: arrays pass through, a base64 string is decoded with Pillow."""
    if isinstance(item, str):
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("a base64 image needs Pillow to be decoded; send uint8 arrays instead") from e
        item = np.array(Image.open(io.BytesIO(base64.b64decode(item))).convert(mode))
    return np.ascontiguousarray(np.asarray(item).astype(np.uint8))


def encode_sparse(mask):
    """[H, W] 0 / 1 -> the [row, col] list of its non-zero entries, row-major (the worker's wire format)."""
    return np.transpose(np.nonzero(mask)).tolist()


class ModelWorker:
    def __init__(self, model, tokenizer, args):
        check_placement(args)
        self.model, self.tokenizer, self.args = model, tokenizer, args
        self.device = model.device_
        if args.load_8bit:                                      # (refused with NotImplementedError where the mode is not built: top-2, adapters, ...)
            model.enable_decode_8bit(True)
        name = args.model_name
        if name is None:                                        # the last path component, or the last two under a checkpoint-N directory
            parts = args.model_path.rstrip("/").split("/")
            name = parts[-2] + "_" + parts[-1] if parts[-1].startswith("checkpoint-") else parts[-1]
        self.model_name = name
        self.is_multimodal = "llava" in name.lower() or "medplib" in name.lower()
        self.context_len = int(getattr(model.config, "max_sequence_length", 2048))       # load_pretrained_model's context_len
        cfg = model.config                                      # 256 / 336 / 14 at the shipped dimensions
        self.sam_img_size, self.clip_img_size = int(getattr(cfg, "sam_image_size", 256)), int(getattr(cfg, "clip_image_size", 336))
        self.patch = int(getattr(cfg, "clip_patch_size", 14))
        self.seg_token_idx = tokenizer("<SEG>", add_special_tokens=False).input_ids[0]

    def get_status(self):
        return {"model_names": [self.model_name], "speed": 1, "queue_length": 0}

    # ---- request -> model inputs
    def _images(self, params):
        """-> (images_clip [1, 3, 336, 336] bf16, images [1, 3, 256, 256] bf16, resize_list, original_size_list) or Nones."""
        images = params.get("images", None)
        if not images or not self.is_multimodal:
            return None, None, None, None
        if len(images) != params["prompt"].count(DEFAULT_IMAGE_TOKEN):
            raise ValueError("Number of images does not match number of <image> tokens in prompt")
        rgb = torch.from_numpy(_as_array(images[0], "RGB")).to(self.device)          # one image per request
        sam, resize = P.preprocess_sam(rgb, self.sam_img_size, out_dtype=torch.bfloat16)
        clip = P.preprocess_clip(rgb, self.clip_img_size, out_dtype=torch.bfloat16)
        return clip.unsqueeze(0), sam.unsqueeze(0), [list(resize)], [tuple(rgb.shape[:2])]

    def _regions(self, params):
        """-> (region_masks, valid_region_masks_bool) in the model's layout: the masks resized and padded like the CLIP image, every 14th
        pixel (nearest at scale 1 / 14: one entry per CLIP patch)."""
        regions = params.get("region_masks", None)
        if not regions:
            return (), ()
        grids = []
        for r in regions:
            m = P.preprocess_region_mask(torch.from_numpy(_as_array(r, "L")).to(self.device), self.clip_img_size)
            grids.append(m[::self.patch, ::self.patch].contiguous())
        return [grids], [[torch.ones(1).bool()]]

    def _request(self, params):
        """One request's params -> what both token loops need: the images and regions, temperature / top_p / top_k, max_new_tokens (capped),
        the stop string and its one-id form, the prompt's ids cut to the context, and a sampling seed from torch's global generator (drawn
        last: requests parsed in list order draw their seeds in list order)."""
        tok = self.tokenizer
        prompt = params["prompt"]
        clip, sam, resize_list, original_size_list = self._images(params)
        if clip is None:
            raise ValueError("a request needs one image: the model's prompt carries the <image> features")
        region_masks, region_valid = self._regions(params)
        temperature = float(params.get("temperature", 1.0))
        top_p = float(params.get("top_p", 1.0))                 # read and never used, as in the reference, unless --apply-top-p
        apply_top_p = bool(getattr(self.args, "apply_top_p", False))
        top_k = int(params.get("top_k", 0)) if apply_top_p else 0
        max_new_tokens = min(int(params.get("max_new_tokens", 256)), MAX_NEW_TOKENS_CAP)
        stop_str = params.get("stop", None)
        stop_idx = None
        if stop_str is not None:                                # a stop string that is ONE id (as the tokenizer returns it) also stops by id
            ids = tok(stop_str).input_ids
            stop_idx = ids[0] if len(ids) == 1 else None
        input_ids = tokenize_with_image_tokens(prompt, tok)     # <image> -> IMAGE_TOKEN_INDEX, region placeholder inside <region></region>
        input_ids = input_ids[-(self.context_len - max_new_tokens - 8):]

        def decode(ids):
            return tok.decode(ids, skip_special_tokens=True)

        def stop_seen(ids):
            return bool(stop_str) and decode(ids).rfind(stop_str) != -1

        return types.SimpleNamespace(
            prompt=prompt, clip=clip, sam=sam, resize_list=resize_list, original_size_list=original_size_list, region_masks=region_masks,
            region_valid=region_valid, temperature=temperature, top_p=top_p, apply_top_p=apply_top_p, top_k=top_k, max_new_tokens=max_new_tokens,
            stop_str=stop_str, stop_idx=stop_idx, input_ids=np.asarray([input_ids], dtype=np.int64), decode=decode, stop_seen=stop_seen,
            seed=int(torch.randint(0, 2 ** 31 - 1, (1,))))

    @staticmethod
    def _message(rq, new_ids, pred_mask):
        """One message of a request: the prompt and the text so far, cut at the last occurrence of the stop string, and the sparse mask."""
        text = rq.decode(new_ids)
        if rq.stop_str:
            pos = text.rfind(rq.stop_str)
            if pos != -1:
                text = text[:pos]
        mask, height, width = [], 0, 0
        if pred_mask is not None:
            m = (torch.sigmoid(pred_mask.float()) > MASK_THRESHOLD).int().squeeze(0).cpu().numpy()
            height, width = m.shape
            mask = encode_sparse(m)
        return json.dumps({"text": rq.prompt + text, "mask": mask, "height": str(height), "width": str(width), "error_code": 0}).encode() + b"\0"

    def _stream_one(self, rq):
        """The messages of one parsed request through the model's generate_stream."""
        for new_ids, stopped, pred_mask in self.model.generate_stream(
                rq.input_ids, rq.clip, images=rq.sam, temperature=rq.temperature, top_p=rq.top_p, max_new_tokens=rq.max_new_tokens,
                stop_token_id=rq.stop_idx, eos_token_id=self.tokenizer.eos_token_id, stream_interval=self.args.stream_interval,
                sample_seed=rq.seed, resize_list=rq.resize_list, original_size_list=rq.original_size_list,
                region_masks=rq.region_masks, valid_region_masks_bool=rq.region_valid, stop_check=rq.stop_seen, top_k=rq.top_k,
                apply_top_p=rq.apply_top_p):
            yield self._message(rq, new_ids, pred_mask)

    @torch.no_grad()
    def generate_stream(self, params):
        yield from self._stream_one(self._request(params))

    @torch.no_grad()
    def generate_stream_batch(self, params_list):
        """The requests a server holds, served together: taken in order in groups of min(8, --limit-model-concurrency), each group the rows
        of one decode step (MedPLIBForCausalLM.generate_stream_batch).  Yields (index in params_list, message bytes); per index the messages
        are generate_stream's: the text cut at the stop string, the sparse mask with the stopping message, the b"\\0" terminator.  All
        requests are parsed first and draw their seeds from torch's global generator in list order.  Where the model refuses batch rows
        (module docstring) the requests are served one after the other through the model's generate_stream, in the same (index, message)
        shape."""
        from medplib_amd.model.generation import StreamRequest
        requests = [self._request(p) for p in params_list]
        if self.model.model.llm.batch_rows_unsupported() is not None:
            for index, rq in enumerate(requests):
                for message in self._stream_one(rq):
                    yield index, message
            return
        rows = max(1, min(8, int(self.args.limit_model_concurrency)))
        for g0 in range(0, len(requests), rows):
            group = requests[g0:g0 + rows]
            batch = [StreamRequest(input_ids=rq.input_ids, images_clip=rq.clip, images=rq.sam, resize_list=rq.resize_list,
                                   original_size_list=rq.original_size_list, region_masks=rq.region_masks,
                                   valid_region_masks_bool=rq.region_valid, temperature=rq.temperature, top_p=rq.top_p, top_k=rq.top_k,
                                   apply_top_p=rq.apply_top_p, max_new_tokens=rq.max_new_tokens, stop_token_id=rq.stop_idx, sample_seed=rq.seed,
                                   stop_check=rq.stop_seen) for rq in group]
            for row, new_ids, stopped, pred_mask in self.model.generate_stream_batch(
                    batch, stream_interval=self.args.stream_interval, eos_token_id=self.tokenizer.eos_token_id):
                yield g0 + row, self._message(group[row], new_ids, pred_mask)

    def generate_stream_gate(self, params):
        yield from self.generate_stream(params)

    def generate_stream_gate_batch(self, params_list):
        yield from self.generate_stream_batch(params_list)
