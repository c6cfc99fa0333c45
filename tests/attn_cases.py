"""Inputs of the flash-attention accuracy tests (CPU tensors; shared by
test_flash_attention_reference.py and test_flash_attention_accuracy_gpu.py).

A case is (qkv bf16 [b, s, 3*nh*64], mask bf16 [b, s] or None,
gy bf16 [b, s, nh*64])."""
import torch

HD = 64
MASKED = -10000.0

REGIMES = ("flat", "peaked", "padding", "general", "fullmask", "spike")


def padding_mask(b, s):
    """Padding that differs per batch: batch i masks its last 7 + 40*i keys;
    batch 0 also masks the whole first 128-key tile (the first tile's
    running max is then ~ -1e4 and the next rescale factor underflows to
    0); the last batch leaves the single key 133 unmasked."""
    mask = torch.zeros(b, s)
    for i in range(b):
        mask[i, s - (7 + 40 * i):] = MASKED
    mask[0, :128] = MASKED
    mask[b - 1] = MASKED
    mask[b - 1, 133] = 0.0
    return mask.bfloat16()


def general_mask(b, s, gen):
    """bf16 values uniform in [-4, 0], independent per batch and key."""
    return (torch.rand(b, s, generator=gen) * -4.0).bfloat16()


def make_case(regime, b, s, nh, seed=0):
    assert regime in REGIMES
    gen = torch.Generator().manual_seed(1000 + seed)
    sigma = 2.0 if regime == "peaked" else 0.5
    qkv = (torch.randn(b, s, 3 * nh * HD, generator=gen) * sigma).bfloat16()
    gy = torch.randn(b, s, nh * HD, generator=gen).bfloat16()
    mask = None
    if regime == "padding":
        mask = padding_mask(b, s)
    elif regime == "general":
        mask = general_mask(b, s, gen)
    elif regime == "fullmask":
        # -10000 on every key of one batch: well defined (softmax is
        # shift-invariant), fp32 handling at |score| ~ 1e4
        mask = torch.zeros(b, s)
        mask[b - 1] = MASKED
        mask = mask.bfloat16()
    elif regime == "spike":
        # a key row of 4.0 in the last tile and |q|: the running max grows
        # late, and the backward recomputes P from an LSE of large magnitude
        qkv5 = qkv.view(b, s, 3, nh, HD)
        qkv5[:, s - 84, 1] = 4.0
        qkv5[:, :, 0] = qkv5[:, :, 0].abs()
    return qkv.contiguous(), mask, gy


def random_keep(b, nh, s, p, gen):
    """A dropout keep tensor [b*nh, s, s]: 1/(1-p) where kept, else 0."""
    kept = torch.rand(b * nh, s, s, generator=gen) >= p
    return kept.float() / (1.0 - p)
