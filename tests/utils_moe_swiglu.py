"""The case table shared by tests/test_moe_gemm_swiglu_cpu.py and
tests/test_moe_gemm_swiglu_gpu.py: the smallest shapes at which the tiles of
_hip/moe_gemm_swiglu.hip can go wrong, with a constructed selection."""
import torch

_G = torch.Generator().manual_seed(11)


def _by_counts(counts, k):
    """topk_idx [T, k] whose experts get exactly these slot counts, the
    slots in a fixed shuffled order"""
    flat = torch.repeat_interleave(torch.arange(len(counts)),
                                   torch.tensor(counts))
    return flat[torch.randperm(flat.numel(), generator=_G)].view(-1, k)


def _many_small():
    """half the slots spread over 128 experts (0 to 3 rows for most), the
    other half on four of them"""
    idx = torch.randint(128, (60, 8), generator=_G)
    idx[30:] = idx[30:] % 4 + 100
    return idx


# name -> (topk_idx [T, k], E, H, I)
CASES = {
    # one K-step and one column tile; empty experts; both sides of a 64-row
    # and of a 128-row boundary
    "ragged": (_by_counts((0, 1, 63, 64, 65, 0, 257, 130), 2), 8, 64, 64),
    # three K-steps; I % 128 = 64, so the backward's ragged column tile must
    # stay out of dw; three forward column tiles
    "odd_tiles": (_by_counts((0, 0, 0, 0, 0, 0, 120, 80), 2), 8, 192, 192),
    "many_small": (_many_small(), 128, 128, 64),
    "one_token": (torch.arange(8).view(1, 8), 8, 64, 128),
}
