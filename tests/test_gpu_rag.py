"""GPU: retrieval of in-context examples (medplib_amd/rag.py, model/rag/image_rag.py) against the executed reference
(tests/golden/rag_reference.*, written by scripts/make_rag_golden.py) and against exact / float64 restatements:
CLIPImageProcessor on the device bit for bit, the exact fp32 top-k, the pooled embedding, the full-depth tower at CLIP-L dims, and the
`build` / `augment` command line end to end."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rag_cases  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "rag_reference.npz")), json.load(open(os.path.join(GOLD, "rag_reference.json")))


@pytest.fixture(scope="module")
def ckpt_dir(gold, tmp_path_factory, dev):
    """The fixture's tiny CLIPVisionModel and CLIP-L-336 preprocessor_config.json, written back out, plus its PNGs."""
    z, doc = gold
    d = tmp_path_factory.mktemp("rag")
    ck = d / "ckpt"
    ck.mkdir()
    flat = rag_cases.unpack_bytes(z["weight_codes"], (-1,), np.int8)
    sd, at = {}, 0
    for name, shape, exp in doc["weights"]:
        n = int(np.prod(shape))
        sd["vision_model." + name] = torch.from_numpy(rag_cases.int8_weight(flat[at:at + n].reshape(shape), exp))
        at += n
    assert at == flat.size
    torch.save(sd, ck / "pytorch_model.bin")
    cfg = dict(doc["tiny_config"], model_type="clip_vision_model", num_channels=3)
    json.dump(cfg, open(ck / "config.json", "w"))
    json.dump(doc["preprocessor_config"], open(ck / "preprocessor_config.json", "w"))
    rag_cases.write_images(str(d / "images"))
    json.dump(doc["candidate_records"], open(d / "cand.json", "w"))
    json.dump(doc["query_records"], open(d / "query.json", "w"))
    return d


# ---------------------------------------------------------------------------------------------------- 1. preprocessing
def _processor_numpy(rgb, s=336, crop=336):
    """CLIPImageProcessor (PIL backend) restated: PIL BICUBIC shortest-edge resize, centre crop, float64 rescale -> float32, normalise."""
    from PIL import Image
    h, w = rgb.shape[:2]
    short, long = (w, h) if w <= h else (h, w)
    nl = int(s * long / short)
    nh, nw = (nl, s) if w <= h else (s, nl)
    r = np.array(Image.fromarray(rgb).resize((nw, nh), Image.BICUBIC)) if (nh, nw) != (h, w) else rgb
    t, l = (nh - crop) // 2, (nw - crop) // 2
    r = r[t:t + crop, l:l + crop]
    x = (r.astype(np.float64) * (1 / 255)).astype(np.float32)
    mean = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)
    std = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)
    return ((x - mean) / std).transpose(2, 0, 1)


def test_processor_bit_equal_to_reference_and_restatement(gold, ckpt_dir, dev):
    from medplib_amd import preprocess as P
    from medplib_amd.rag import load_rgb, processor_settings
    z, doc = gold
    st = processor_settings(str(ckpt_dir / "ckpt"))
    delta = rag_cases.unpack_bytes(z["pixel_codes_delta"], doc["pixel_values_shape"], np.uint8)
    pixel_values = rag_cases.unpack_pixel_values(z["pixel_table"], delta)
    for i, name in enumerate(doc["image_names"]):
        rgb = load_rgb(str(ckpt_dir / "images" / name))
        out = P.preprocess_clip_processor(torch.from_numpy(rgb).to(dev), out_dtype=torch.float32, **st).cpu().numpy()
        assert np.array_equal(out.view(np.uint32), pixel_values[i].view(np.uint32)), name
        assert np.array_equal(out, _processor_numpy(rgb)), name
    rng = np.random.default_rng(3)
    for _ in range(14):
        h, w = (int(v) for v in rng.integers(17, 1501, 2))
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out = P.preprocess_clip_processor(torch.from_numpy(rgb).to(dev), out_dtype=torch.float32, **st).cpu().numpy()
        assert np.array_equal(out, _processor_numpy(rgb)), (h, w)
        bf = P.preprocess_clip_processor(torch.from_numpy(rgb).to(dev), out_dtype=torch.bfloat16, **st)
        assert torch.equal(bf, torch.from_numpy(out).to(dev).to(torch.bfloat16))
    with pytest.raises(NotImplementedError, match="resample"):
        P.preprocess_clip_processor(torch.from_numpy(rgb).to(dev), resample=2)


# ---------------------------------------------------------------------------------------------------- 2-3. dot_topk
def _expected_topk(index, queries, k):
    s = queries.astype(np.float64) @ index.astype(np.float64).T          # exact here: entries in {0, +-1, +-1/2, +-1/4}
    N = index.shape[0]
    out_s = np.full((queries.shape[0], k), -np.inf, np.float32)
    out_i = np.full((queries.shape[0], k), -1, np.int32)
    for q in range(queries.shape[0]):
        order = np.lexsort((np.arange(N), -s[q]))[:k]                  # descending score, ties to the lower index
        out_s[q, :len(order)] = s[q, order]
        out_i[q, :len(order)] = order
    return out_s, out_i


def test_dot_topk_exact(dev):
    from medplib_amd import ops
    rng = np.random.default_rng(0)
    vals = np.array([0, 0, 0, 1, -1, 0.5, -0.5, 0.25, -0.25], np.float32)
    C = 64
    for N in (1, 63, 65, 100003):
        index = rng.choice(vals, (N, C)).astype(np.float32)
        if N > 10:
            index[N // 2] = index[3]                                   # duplicate rows: exact ties
            index[N - 1] = index[3]
        for Q in (1, 7, 333):
            queries = rng.choice(vals, (Q, C)).astype(np.float32)
            queries[Q // 2] = 0                                        # a zero query: every score ties at 0
            if N > 10:
                queries[0] = index[3]
            di, dq = torch.from_numpy(index).to(dev), torch.from_numpy(queries).to(dev)
            for k in (1, 3, 16, 64):
                es, ei = _expected_topk(index, queries, k)
                s, i = ops.dot_topk(di, dq, k)
                s, i = s.cpu().numpy(), i.cpu().numpy()
                assert np.array_equal(i, ei), (N, Q, k)
                assert np.array_equal(s, es), (N, Q, k)
                if k > N:
                    assert (i[:, N:] == -1).all() and np.isneginf(s[:, N:]).all()


def test_dot_topk_strided_index(dev):
    from medplib_amd import ops
    rng = np.random.default_rng(1)
    vals = np.array([0, 1, -1, 0.5, -0.5], np.float32)
    big = torch.from_numpy(rng.choice(vals, (1000, 132)).astype(np.float32)).to(dev)
    index = big[:, :128]                                               # row stride 132
    q = torch.from_numpy(rng.choice(vals, (5, 128)).astype(np.float32)).to(dev)
    for Q in (1, 5):
        es, ei = _expected_topk(index.cpu().numpy(), q[:Q].cpu().numpy(), 8)
        s, i = ops.dot_topk(index, q[:Q], 8)
        assert np.array_equal(i.cpu().numpy(), ei) and np.array_equal(s.cpu().numpy(), es)


def test_dot_topk_random_unit_vectors(dev):
    from medplib_amd import ops
    g = torch.Generator(device=dev).manual_seed(7)
    Q, N, C, k = 64, 200_000, 1024, 16
    index = torch.nn.functional.normalize(torch.randn(N, C, generator=g, device=dev), dim=1)
    queries = torch.nn.functional.normalize(torch.randn(Q, C, generator=g, device=dev), dim=1)
    queries[1:8] = index[100:107] + 0.01 * queries[1:8]                 # a few queries with a clear nearest neighbour
    s64 = queries.double() @ index.double().T
    bound = 1.5e-7 * (queries.double().abs() @ index.double().abs().T)
    for qs in (queries, queries[:1]):
        s, i = ops.dot_topk(index, qs, k)
        il = i.long()
        ref = s64[:qs.shape[0]].gather(1, il)
        err = (s.double() - ref).abs() / (bound[:qs.shape[0]].gather(1, il) / 1.5e-7)
        print(f"dot_topk Q={qs.shape[0]}: max |score - float64| / sum|a b| = {float(err.max()):.3e}")   # measured: 1.40e-7 / 2.2e-8
        assert (err <= 1.5e-7).all()
        assert (s[:, :-1] >= s[:, 1:]).all()
        top = s64[:qs.shape[0]].topk(k, dim=1)
        kth = top.values[:, -1:]
        for q in range(qs.shape[0]):
            got, want = set(i[q].tolist()), set(top.indices[q].tolist())
            for c in got ^ want:                                       # only near-ties of the k-th score may swap
                assert abs(float(s64[q, c] - kth[q, 0])) <= 2 * float(bound[q, c]), (q, c)


# ---------------------------------------------------------------------------------------------------- 4. pooled embedding
def test_clip_pool_normalize_against_float64(dev):
    from medplib_amd import ops
    n, S, C = 3, 577, 1024
    g = torch.Generator(device=dev).manual_seed(2)
    x = (torch.randn(n * S, C, generator=g, device=dev) * 2 + 0.3).to(torch.bfloat16)
    out = ops.clip_pool_normalize(x, n).double().cpu()
    m64 = x.double().cpu().view(n, S, C)[:, 1:].mean(1)
    mb = m64.float().to(torch.bfloat16)
    ulp_bf = (mb.float().abs() * 2.0 ** -7).double().clamp_min(2.0 ** -133)
    got_m = (out * mb.double().norm(dim=1, keepdim=True)).float().to(torch.bfloat16)   # our bf16 mean, recovered from the output
    assert ((got_m.double() - m64).abs() <= ulp_bf + (mb.double() - m64).abs()).all()
    assert ((got_m.double() - mb.double()).abs() <= ulp_bf).all()
    want = got_m.double() / (got_m.double().norm(dim=1, keepdim=True) + 1e-12)
    ulp = want.float().abs().double() * 2.0 ** -23
    assert ((out - want).abs() <= 2 * ulp + 1e-30).all()
    rows = torch.randn(37, 1024, generator=g, device=dev)
    y = ops.l2_normalize_rows(rows).double().cpu()
    w = rows.double().cpu() / (rows.double().cpu().norm(dim=1, keepdim=True) + 1e-12)
    assert ((y - w).abs() <= 2 * w.float().abs().double() * 2.0 ** -23 + 1e-30).all()


# ---------------------------------------------------------------------------------------------------- 5. full-depth tower
def test_encode_pooled_full_depth_clip_l(dev, tmp_path):
    from medplib_amd.model.clip import ClipTower
    from medplib_amd.model.config import MedPLIBConfig
    from oracle import llm
    cfg = MedPLIBConfig(hidden_size=64, intermediate_size=64, mm_vision_select_layer=24)
    C, I, ps = cfg.clip_hidden_size, cfg.clip_intermediate_size, cfg.clip_patch_size
    g = torch.Generator().manual_seed(11)

    def rn(*shape, s):
        return (torch.randn(*shape, generator=g) * s).to(torch.bfloat16).float()
    tp = "vision_model."
    W = {tp + "embeddings.patch_embedding.weight": rn(C, 3, ps, ps, s=0.03), tp + "embeddings.class_embedding": rn(C, s=0.5),
         tp + "embeddings.position_embedding.weight": rn(cfg.clip_num_patches + 1, C, s=0.1),
         tp + "pre_layrnorm.weight": 1 + rn(C, s=0.1), tp + "pre_layrnorm.bias": rn(C, s=0.1)}
    for i in range(cfg.clip_num_layers):
        lp = f"{tp}encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            W[lp + n + ".weight"] = 1 + rn(C, s=0.1); W[lp + n + ".bias"] = rn(C, s=0.1)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            W[lp + f"self_attn.{n}.weight"] = rn(C, C, s=C ** -0.5); W[lp + f"self_attn.{n}.bias"] = rn(C, s=0.05)
        W[lp + "mlp.fc1.weight"] = rn(I, C, s=C ** -0.5); W[lp + "mlp.fc1.bias"] = rn(I, s=0.05)
        W[lp + "mlp.fc2.weight"] = rn(C, I, s=I ** -0.5); W[lp + "mlp.fc2.bias"] = rn(C, s=0.05)
    images = torch.randn(2, 3, 336, 336, generator=g).to(torch.bfloat16)
    tower = ClipTower(cfg, dev)
    tower.load_hf(W, tower_prefix=tp, proj_prefix=None)
    got = tower.encode_pooled(images.to(dev)).double().cpu()
    with torch.no_grad():
        Wd = {k: v.to(dev) for k, v in W.items()}
        feats = llm.clip_features(images.float().to(dev), Wd, cfg, prefix=tp).double().cpu()    # fp32 oracle, hidden_states[24][:, 1:]
    m = feats.mean(1)
    ref = m / (m.norm(dim=1, keepdim=True) + 1e-12)
    cos = (got * ref).sum(1) / (got.norm(dim=1) * ref.norm(dim=1))
    print("encode_pooled vs fp32 oracle, CLIP-L 24 layers, cosine per image:", cos.tolist())
    # measured on the MI355X: 0.9999971 and 0.9999970 (bf16 tower against the fp32 oracle, 24 layers, CLIP-L dims)
    assert (cos >= 0.9995).all(), cos.tolist()


# ---------------------------------------------------------------------------------------------------- 6-8. command line end to end
def _run_cli(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "model", "rag", "image_rag.py")] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _common(d, index_dir, bs=16):
    return ["--rag_encoder_path", str(d / "ckpt"), "--image_folder", str(d / "images"), "--index_dir", str(index_dir),
            "--batch_size", str(bs)]


_BUILD_LINES = {}


@pytest.fixture(scope="module")
def cli_runs(ckpt_dir, dev):
    d = ckpt_dir
    out = _BUILD_LINES
    for bs in (16, 5):
        idx = d / f"index{bs}"
        out[f"build{bs}"] = _run_cli(["build"] + _common(d, idx, bs) + ["--candidate_json", str(d / "cand.json")])
        _run_cli(["augment"] + _common(d, idx, bs) + ["--query_json", str(d / "query.json"), "--output_json",
                                                      str(d / f"out{bs}" / "aug.json"), "--top_k", "3"])
    return d


def test_cli_build_and_augment_match_reference(gold, cli_runs, dev):
    from medplib_amd.rag import ImageRAGEncoder, extract_query_image, resolve_path
    z, doc = gold
    d = cli_runs
    assert _BUILD_LINES["build16"].strip() == doc["build_line"].replace("<index_dir>", str(d / "index16"))
    assert open(d / "index16" / "metadata.json").read() == doc["metadata_json"]
    emb = np.load(d / "index16" / "embeddings.npy")
    ref = z["embeddings"]
    assert emb.dtype == np.float32 and emb.shape == ref.shape
    cos = (emb * ref).sum(1) / (np.linalg.norm(emb, axis=1) * np.linalg.norm(ref, axis=1))
    print("index rows vs the reference's fp32 embeddings, cosine:", cos.tolist())     # measured: >= 0.999998 on every row
    assert (cos >= 0.999).all(), cos.tolist()
    # delta: 4 x the largest score difference between this build's and the reference's embeddings
    enc = ImageRAGEncoder("clip_encoder", str(d / "ckpt"))
    qf = enc.encode_paths([resolve_path(extract_query_image(it), str(d / "images")) for it in doc["query_records"]])
    idx_dev = emb / (np.linalg.norm(emb, axis=1, keepdims=True) + 1e-12)
    delta = 4 * float(np.abs(qf.astype(np.float64) @ idx_dev.T.astype(np.float64) - z["scores"]).max())
    print("augment delta (4 x max |score difference|):", delta)                        # measured: 0.00105
    assert delta <= 0.01
    meta = json.loads(doc["metadata_json"])
    ours, theirs = json.load(open(d / "out16" / "aug.json")), json.loads(doc["augmented_json"])
    assert len(ours) == len(theirs)
    for qi, (a, b) in enumerate(zip(ours, theirs)):
        assert {k: v for k, v in a.items() if k != "icl_examples"} == {k: v for k, v in b.items() if k != "icl_examples"}
        assert len(a["icl_examples"]) == len(b["icl_examples"]) == 3
        sc = z["scores"][qi]
        ga = [meta.index(e) for e in a["icl_examples"]]
        gb = [meta.index(e) for e in b["icl_examples"]]
        for p, (x, y) in enumerate(zip(ga, gb)):
            if x != y:                                                  # exact ties (|difference| 0) and near ties only
                assert abs(float(sc[x]) - float(sc[y])) <= delta, (qi, p, x, y)
        for x in ga:                                                    # tie groups are compared as groups: equal scores, lower row first
            tied = [j for j in range(len(meta)) if sc[j] == sc[x]]
            assert [j for j in ga if j in tied] == sorted(j for j in ga if j in tied)


def test_batch_size_independence(cli_runs):
    d = cli_runs
    a16 = open(d / "out16" / "aug.json").read()
    a5 = open(d / "out5" / "aug.json").read()
    assert a16 == a5
    e16, e5 = np.load(d / "index16" / "embeddings.npy"), np.load(d / "index5" / "embeddings.npy")
    print("embeddings with --batch_size 16 and 5 bitwise equal:", bool(np.array_equal(e16.view(np.uint32), e5.view(np.uint32))),
          "max |diff|", float(np.abs(e16 - e5).max()))
    # within 1 bf16 ulp of the mean, carried through the normalisation (|row| = 1)
    assert (np.abs(e16 - e5) <= np.abs(e16) * 2.0 ** -7 + 1e-7).all()


def test_augmented_json_feeds_the_icl_dataset(cli_runs):
    from datasets import ICLLazySupervisedDataset
    from medplib_amd.dataset import icl_examples_of
    d = cli_runs
    data_args = types.SimpleNamespace(image_folder=str(d / "images"), image_processor=None)
    ds = ICLLazySupervisedDataset(str(d / "out16" / "aug.json"), None, data_args)
    aug = json.load(open(d / "out16" / "aug.json"))
    assert len(ds) == len(aug)
    for i, rec in enumerate(aug):
        assert icl_examples_of(ds.records[i]) == rec["icl_examples"][:3]
        assert ds.records[i]["image"] == rec["image"]
