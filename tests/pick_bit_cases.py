"""Inputs and runners of the bit-exactness test of the three row-pick kernels (no test in here): mp_sample_rows_f32,
mp_sample_filtered_rows_f32 and mp_beam_topk_f32 on the smallest shapes at which a change of their fp32 summation order, piece layout or
tie rule would show.  scripts/record_pick_bits.py runs `results` on the device and stores them, with a SHA-256 of every generated input, in
tests/golden/pick_bits.npz; tests/test_gpu_pick_bits.py runs `results` again and compares byte for byte."""
import functools
import hashlib

import numpy as np
import torch

from beam_cases import beam_case
from medplib_amd import ops
from test_gpu_sample import BELOW_ONE, _uniforms

# a piece straddling `cols`, cols no multiple of 4, one wave / many waves, the last <8, true> width and the first <16, false> one
COLS = (2, 63, 64, 1000, 4099, 32011, 32768, 32769, 65536)
TEMPS = (0.2, 0.7, 1.0)
CONTENTS = ("normal", "tie3", "neg_inf_runs", "nan", "all_neg_inf", "all_nan")
N_U = 19                                    # per (row, T): 0, BELOW_ONE, 1.0 and 16 of test_gpu_sample._uniforms' points
BATCH_U = (0, 1, 2, 5, 10, 15)              # the batches are launched once per entry: row r draws its own u[..., j]
LAYOUTS = ("ld0", "ld_cols", "ld_cols3")    # one row against every u; 5 rows at ld = cols (odd cols: rows off 16 bytes); 5 rows at ld = cols + 3
BEAM_NBS = (1, 2, 4, 8)
BEAM_COLS = COLS[1:]


def filters(cols):
    return ((0, 1.0), (cols + 5, 1.0), (1, 1.0), (50, 1.0), (0, 0.9), (50, 0.9), (0, 0.0), (0, 1e-6), (cols - 1, 0.999))


def _cdf64(row, T):
    """The float64 CDF the u are placed on: NaN and -inf columns weigh 0; a row without a finite column gets a uniform one."""
    l = row.astype(np.float64)
    ok = np.isfinite(l)
    if not ok.any():
        return np.linspace(1.0 / len(l), 1.0, len(l))
    w = np.where(ok, np.exp((np.where(ok, l, 0.0) - l[ok].max()) / T), 0.0)
    c = np.cumsum(w)
    return c / c[-1]


@functools.lru_cache(maxsize=None)
def sampling_inputs(cols):
    """-> (rows fp32 [6, cols] in CONTENTS order, u fp32 [6, len(TEMPS), N_U]), seeded by cols."""
    g = torch.Generator().manual_seed(1000 + cols)
    inf, nan = float("inf"), float("nan")
    rows = torch.randn(len(CONTENTS), cols, generator=g) * 3
    rows[1, [cols // 5, cols // 2, cols - 1]] = float(rows[1].max()) + 1.0          # (cols = 2: a two-way tie)
    if cols == 2:
        rows[2, 1] = -inf
    else:
        rows[2, 0] = -inf
        rows[2, cols // 4:cols // 2] = -inf
        rows[2, cols - cols // 8 - 1:] = -inf
    rows[3, 5::7] = nan
    rows[3, -1] = nan
    rows[4] = -inf
    rows[5] = nan
    rows = rows.numpy()
    u = np.empty((len(CONTENTS), len(TEMPS), N_U), dtype=np.float32)
    for r in range(len(CONTENTS)):
        for t, T in enumerate(TEMPS):
            points = _uniforms(_cdf64(rows[r], T), 16, g)[4:]                      # next to steps of the CDF, and random ones
            u[r, t] = np.concatenate([[0.0, BELOW_ONE, 1.0], points[np.linspace(0, len(points) - 1, 16).astype(np.int64)]])
    return rows, u


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def _sampling_launches(cols, dev):
    """Yields (layout, T, logits view on the device, u on the device) for every launch shape of one width."""
    rows, u = sampling_inputs(cols)
    rows_d, u_d = torch.from_numpy(rows).to(dev), torch.from_numpy(u).to(dev)
    batches = {}
    for layout, pad, fifth in (("ld_cols", 0, 4), ("ld_cols3", 3, 5)):
        back = torch.full((5, cols + pad), 1e30, device=dev)                       # (the columns between the rows are never read)
        pick = [0, 1, 2, 3, fifth]
        back[:, :cols] = rows_d[pick]
        batches[layout] = (back[:, :cols], pick)
    for t, T in enumerate(TEMPS):
        for r in range(len(CONTENTS)):
            yield "ld0", T, rows_d[r].view(1, cols).expand(N_U, cols), u_d[r, t].contiguous()
        for layout, (view, pick) in batches.items():
            for j in BATCH_U:
                yield layout, T, view, u_d[pick, t, j].contiguous()


def _tokens16(parts):
    tok = torch.cat(parts).cpu().numpy()
    assert tok.min() >= 0 and tok.max() < 65536
    return tok.astype(np.uint16)


def input_hashes():
    out = {f"sha/sampling/{cols}": _sha(*sampling_inputs(cols)) for cols in COLS}
    for nb in BEAM_NBS:
        out[f"sha/beam/{nb}"] = _sha(*[a.numpy() for case in _beam_cases(nb) for a in (case[0], case[2])])
    return out


def plain_results(dev):
    """name -> array: the tokens of mp_sample_rows_f32, per (cols, layout) over T, rows / launches and u."""
    out = {}
    for cols in COLS:
        parts = {layout: [] for layout in LAYOUTS}
        for layout, T, view, u in _sampling_launches(cols, dev):
            parts[layout].append(ops.sample_rows(view, u, T))
        for layout in LAYOUTS:
            out[f"plain/{cols}/{layout}"] = _tokens16(parts[layout])
    return out


def filtered_results(dev):
    """name -> array: tokens without want_cut, and tokens, kept and cut (as uint32) with it, of mp_sample_filtered_rows_f32."""
    out = {}
    for cols in COLS:
        parts = {layout: ([], [], [], []) for layout in LAYOUTS}
        for layout, T, view, u in _sampling_launches(cols, dev):
            for k, p in filters(cols):
                tok, kept, cut = ops.sample_rows_filtered(view, u, T, k, p, want_cut=True)
                for lst, a in zip(parts[layout], (ops.sample_rows_filtered(view, u, T, k, p), tok, kept, cut)):
                    lst.append(a)
        for layout in LAYOUTS:
            tok, tok_cut, kept, cut = parts[layout]
            out[f"filtered/{cols}/{layout}/tokens"] = _tokens16(tok)
            out[f"filtered/{cols}/{layout}/tokens_want_cut"] = _tokens16(tok_cut)
            out[f"filtered/{cols}/{layout}/kept"] = torch.cat(kept).cpu().numpy()
            out[f"filtered/{cols}/{layout}/cut"] = torch.cat(cut).cpu().numpy().view(np.uint32)
    return out


def _beam_cases(nb):
    """(backing logits, view [nb or 1, cols], scores, eos) per (cols, ld, scores, eos): eos = -1, and the best token of beam 0, the beam with
    the highest score: a candidate inside the top nb (the recorder checks that) which the selection then skips."""
    for cols in BEAM_COLS:
        for ld in ("cols", "zero"):
            for scores in ("first", "spread"):
                back, view, s = beam_case(nb, cols, ld, scores, 0)
                for eos in (-1, int(view[0].argmax())):
                    yield back, view, s, eos


def beam_results(dev):
    """name -> array: every output of mp_beam_topk_f32 (scores as uint32), per nb over the cases of _beam_cases."""
    out = {}
    for nb in BEAM_NBS:
        names = ("cand_score", "cand_index", "next_scores", "next_tokens", "next_parent", "err")
        parts = {n: [] for n in names}
        for back, view, s, eos in _beam_cases(nb):
            o = {"cand_score": torch.full((2 * nb,), 7.0, device=dev), "cand_index": torch.full((2 * nb,), -7, dtype=torch.int32, device=dev),
                 "next_scores": torch.full((nb,), 7.0, device=dev), "next_tokens": torch.full((nb,), -7, dtype=torch.int64, device=dev),
                 "next_parent": torch.full((nb,), -7, dtype=torch.int32, device=dev), "err": torch.zeros(1, dtype=torch.int32, device=dev)}
            ops.beam_topk(back.to(dev)[:, :view.shape[1]], s.to(dev), eos, o["cand_score"], o["cand_index"], o["next_scores"], o["next_tokens"],
                          o["next_parent"], o["err"], nb=nb)
            for n in names:
                parts[n].append(o[n])
        for n in names:
            a = torch.cat(parts[n]).cpu().numpy()
            out[f"beam/{nb}/{n}"] = a.view(np.uint32) if a.dtype == np.float32 else a
    return out


def results(dev):
    return {**input_hashes(), **plain_results(dev), **filtered_results(dev), **beam_results(dev)}
