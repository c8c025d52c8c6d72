"""Records tests/golden/pick_bits.npz: what mp_sample_rows_f32, mp_sample_filtered_rows_f32 and mp_beam_topk_f32 return, bit for bit, on
the inputs of tests/pick_bit_cases.py, with a SHA-256 of every generated input.  Run it on the GPU at the commit whose bits are the
standard (the parent of a change that must not move them); tests/test_gpu_pick_bits.py then holds every later tree to the file.
python scripts/record_pick_bits.py [--out tests/golden/pick_bits.npz]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import pick_bit_cases as cases

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pick_bits.npz"))
args = ap.parse_args()
dev = torch.device("cuda:0")
res = cases.results(dev)
again = cases.results(dev)
assert all(np.array_equal(res[k], again[k]) for k in res), "two runs on one tree differ: nothing to record"
for nb in cases.BEAM_NBS:                  # every second case carries an eos: it must be a candidate inside the top nb, and never selected
    cand = res[f"beam/{nb}/cand_index"].reshape(-1, 2 * nb)
    nxt = res[f"beam/{nb}/next_tokens"].reshape(-1, nb)
    for i, (_, view, _, eos) in enumerate(cases._beam_cases(nb)):
        assert eos < 0 or (eos in (cand[i, :nb] % view.shape[1]) and eos not in nxt[i]), (nb, i, eos)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
np.savez_compressed(args.out, **res)
print(f"{args.out}: {len(res)} arrays, {sum(a.nbytes for a in res.values())} bytes of results, {os.path.getsize(args.out)} bytes on disk")
