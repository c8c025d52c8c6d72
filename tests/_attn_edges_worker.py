"""Worker of tests/test_gpu_attention_edges.py::test_ab_forms_of_the_v2_kernel: the forward length sweep and the mask cases for variant 0,
both head sizes, with the bounds of the parent test, in a process whose MP_ATTN_* setting the parent chose (the library reads them once)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402


def main():
    import test_gpu_attention_edges as T
    dev = torch.device("cuda", 0)
    print("settings:", {k: v for k, v in os.environ.items() if k.startswith("MP_ATTN_")})
    for D in (64, 128):
        T.run_length_sweep(dev, 0, D)
        T.run_mask_cases(dev, 0, D)
    torch.cuda.synchronize()
    T._show("fwd")
    print("attn-edges-worker ok")


if __name__ == "__main__":
    main()
