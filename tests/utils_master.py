"""Shared by tests/test_master_weights_cpu.py and
tests/test_master_weights_gpu.py: bit views and the stall scenario.  A plain
module like tests/utils_numerics.py, not a conftest."""
import torch

from distributed_training_guide_amd.ops import FusedAdamW, split_master


def bits(u):
    """fp32 tensor from a list / tensor of 32-bit patterns (0..2^32-1)."""
    u = torch.as_tensor(u, dtype=torch.int64)
    return ((u + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).view(
        torch.float32)


def i32(x):
    return x.contiguous().view(torch.int32)


def i16(x):
    return x.contiguous().view(torch.int16)


def set_grad(p, g):
    if g.dtype != p.dtype:
        p.grad_dtype = g.dtype
    p.grad = g


def stall_setup(n=4096, seed=0):
    """(start bf16 values, gradient of step s): randn * 0.02 parameters,
    fixed-sign gradients of about 1e-3, as bf16."""
    g = torch.Generator().manual_seed(seed)
    w0 = (torch.randn(n, generator=g) * 0.02).bfloat16()
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)

    def grad(s):
        gs = torch.Generator().manual_seed(1000 + s)
        return (sign * 1e-3 * (1.0 + 0.1 * torch.rand(n, generator=gs))) \
            .bfloat16()
    return w0, grad


def run_stall(device, steps):
    """lr 3e-5, no weight decay, bf16 gradients, three optimizers on
    `device`: a master-weight bf16 parameter, the same start values as an
    fp32 parameter, and a plain bf16 parameter.  After every step the master
    is bit-equal to the fp32 parameter and the visible bf16 tensor is the
    bf16 half of its split.  Returns the fractions of elements with
    |w| >= 2^-6 that still show their start value: (master, plain)."""
    w0, grad = stall_setup()
    w0 = w0.to(device)
    pb = torch.nn.Parameter(w0.clone())
    pf = torch.nn.Parameter(w0.float())
    plain = torch.nn.Parameter(w0.clone())
    kw = dict(lr=3e-5, weight_decay=0.0)
    ob = FusedAdamW([pb], master_weights=True, **kw)
    of = FusedAdamW([pf], **kw)
    op = FusedAdamW([plain], **kw)
    for s in range(steps):
        g = grad(s).to(device)
        pb.grad = g.clone()
        set_grad(pf, g.clone())
        plain.grad = g.clone()
        ob.step()
        of.step()
        op.step()
        assert torch.equal(i32(ob.master_param(pb)), i32(pf.detach())), s
        assert torch.equal(i16(pb.detach()),
                           i16(split_master(pf.detach())[0])), s
    lo = ob.state[pb]["master_lo"]
    assert lo.dtype == torch.int16 and lo.ne(0).any()
    big = w0.float().abs() >= 2.0 ** -6
    assert big.sum() > 1000
    frozen = (pb.detach() == w0)[big].float().mean().item()
    frozen_plain = (plain.detach() == w0)[big].float().mean().item()
    return frozen, frozen_plain
