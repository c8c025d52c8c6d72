"""The NF4 decode-weight format restated in torch on the CPU (no import from medplib_amd): the sixteen-entry table of QLoRA, the fifteen
decision thresholds, the block-wise quantiser, the pack order and the dequantisation with the bf16-rounded table the GEMV multiplies with.

A weight is a 4-bit code; 64 consecutive k of a row share one fp32 absmax; byte j of a row is code[2j] << 4 | code[2j + 1]."""
import torch

BLOCK = 64

# fp32 literals of the table: float(repr) round trips, and the tensor below holds them exactly
NF4 = torch.tensor([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
                    -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
                    0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0], dtype=torch.float32)

# T[i] = fp32(((double)NF4[i] + (double)NF4[i + 1]) / 2): a value strictly above T[i] has a code above i
THRESHOLDS = ((NF4[:-1].double() + NF4[1:].double()) / 2).float()

# the table as the GEMV multiplies with it: rounded to bf16, nearest even (held in fp32)
NF4_BF16 = NF4.to(torch.bfloat16).float()


def quant_codes(w):
    """w [..., K] (K % 64 == 0) -> (code uint8 [..., K] one per weight, absmax fp32 [..., K/64]); every step one fp32 operation."""
    f = w.float()
    assert f.shape[-1] % BLOCK == 0
    blocks = f.unflatten(-1, (-1, BLOCK))
    absmax = blocks.abs().amax(-1)
    inv = torch.where(absmax > 0, torch.tensor(1.0) / absmax, torch.zeros_like(absmax))
    v = blocks * inv.unsqueeze(-1)
    code = (v.unsqueeze(-1) > THRESHOLDS).sum(-1).to(torch.uint8)          # strict: a tie goes to the lower code
    return code.flatten(-2), absmax


def pack(code):
    """code uint8 [..., K] -> bytes uint8 [..., K/2]: the even k is the high nibble."""
    return (code[..., 0::2] << 4) | code[..., 1::2]


def unpack(packed):
    """bytes uint8 [..., K/2] -> code uint8 [..., K]."""
    return torch.stack((packed >> 4, packed & 15), dim=-1).flatten(-2)


def quant_ref(w):
    """The quantiser: w [..., K] bf16 -> (codes uint8 [..., K/2] packed, absmax fp32 [..., K/64])."""
    code, absmax = quant_codes(w)
    return pack(code), absmax


def dequant_ref(codes, absmax, table=NF4_BF16):
    """(packed codes, absmax) -> fp32 [..., K]: table[code] * absmax, one fp32 product per weight, with the bf16-rounded table."""
    code = unpack(codes.cpu()).long()
    return table[code] * absmax.cpu().float().repeat_interleave(BLOCK, dim=-1)
