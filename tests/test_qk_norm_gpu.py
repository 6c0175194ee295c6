"""qkv_norm_rope.hip on the GPU: the bindings against fp64 per element,
run-to-run determinism, argument checks, and qwen3-debug through the kernel
path (bf16 against the CPU fp32 model, convergence, FP8 linears)."""
import functools

import pytest
import torch

from utils_numerics import rope_positions
from utils_qk_norm import (EPS, MAX_POS, SHAPES, assert_qk_close, qk_inputs,
                           qk_ref64, tables)

pytestmark = pytest.mark.gpu

# The forward launcher caps its grid at 1024 blocks of 4 waves, one token
# per wave per step: with B = 1 the grid-stride loop wraps from S = 4097 on
# (the backward's cap of 768 blocks wraps earlier).  Smallest such S at
# Hq 8, Hkv 2, D 128; its table is sized to it.
WRAP_SHAPE = (1, 4 * 1024 + 1, 8, 2, 128)


def _ext():
    from distributed_training_guide_amd._ext import ext

    return ext()


@functools.lru_cache(maxsize=None)
def _case(shape, with_positions):
    """Inputs, tables, positions and the fp64 reference on the GPU, once per
    (shape, positions); no test modifies them."""
    B, S, Hq, Hkv, D = shape
    inp = qk_inputs(B, S, Hq, Hkv, D, device="cuda")
    max_pos = max(MAX_POS, S + 16)
    cos, sin = tables(D, max_pos, "cuda")
    pos = rope_positions(S, max_pos, "cuda") if with_positions else None
    return inp, cos, sin, pos, qk_ref64(inp, Hq, Hkv, D, cos, sin, pos)


def _run(inp, cos, sin, pos, Hq, Hkv, D):
    C = _ext()
    q, k, v = C.qkv_norm_rope_fwd(inp["qkv"], inp["wq"], inp["wk"], cos, sin,
                                  pos, Hq, Hkv, D, EPS)
    dqkv, dwq, dwk = C.qkv_norm_rope_bwd(inp["dq"], inp["dk"], inp["dv"],
                                         inp["qkv"], inp["wq"], inp["wk"],
                                         cos, sin, pos, EPS)
    return dict(q=q, k=k, v=v, dqkv=dqkv, dwq=dwq, dwk=dwk)


@pytest.mark.parametrize("with_positions", [False, True])
@pytest.mark.parametrize("shape", SHAPES + (WRAP_SHAPE,))
def test_bindings_match_fp64(shape, with_positions):
    B, S, Hq, Hkv, D = shape
    inp, cos, sin, pos, ref = _case(shape, with_positions)
    got = _run(inp, cos, sin, pos, Hq, Hkv, D)
    assert got["q"].shape == (B, S, Hq, D)
    assert got["k"].shape == got["v"].shape == (B, S, Hkv, D)
    assert got["dqkv"].shape == inp["qkv"].shape
    assert got["dwq"].shape == got["dwk"].shape == (D,)
    assert_qk_close(got, ref, f"{shape} pos={with_positions}")
    assert torch.equal(got["dqkv"][..., (Hq + Hkv) * D:],
                       inp["dv"].reshape(B, S, Hkv * D))


@pytest.mark.parametrize("shape", [SHAPES[1], WRAP_SHAPE])
def test_backward_is_deterministic(shape):
    B, S, Hq, Hkv, D = shape
    inp, cos, sin, pos, _ = _case(shape, True)
    a = _run(inp, cos, sin, pos, Hq, Hkv, D)
    b = _run(inp, cos, sin, pos, Hq, Hkv, D)
    for key in ("dwq", "dwk", "dqkv"):
        assert torch.equal(a[key], b[key]), key


def test_autograd_op_matches_bindings():
    """ops.qkv_norm_rope on the GPU is the two bindings under autograd."""
    from distributed_training_guide_amd.ops import qkv_norm_rope
    from utils_qk_norm import THETA

    shape = SHAPES[2]
    B, S, Hq, Hkv, D = shape
    inp, cos, sin, _, ref = _case(shape, False)
    qkv = inp["qkv"].clone().requires_grad_(True)
    wq = inp["wq"].clone().requires_grad_(True)
    wk = inp["wk"].clone().requires_grad_(True)
    q, k, v = qkv_norm_rope(qkv, wq, wk, Hq, Hkv, D, EPS, theta=THETA,
                            max_pos=MAX_POS)
    torch.autograd.backward([q, k, v], [inp["dq"], inp["dk"], inp["dv"]])
    got = dict(q=q.detach(), k=k.detach(), v=v.detach(), dqkv=qkv.grad,
               dwq=wq.grad, dwk=wk.grad)
    assert_qk_close(got, ref, "autograd op")
    with pytest.raises(ValueError, match="head dim 32"):
        qkv_norm_rope(torch.zeros(1, 4, 4 * 32, device="cuda",
                                  dtype=torch.bfloat16),
                      torch.ones(32, device="cuda", dtype=torch.bfloat16),
                      torch.ones(32, device="cuda", dtype=torch.bfloat16),
                      2, 1, 32, EPS)


def test_argument_checks():
    C = _ext()
    shape = SHAPES[1]
    B, S, Hq, Hkv, D = shape
    inp, cos, sin, pos, ref = _case(shape, True)
    qkv, wq, wk = inp["qkv"], inp["wq"], inp["wk"]
    dq, dk, dv = inp["dq"], inp["dk"], inp["dv"]

    def fwd(qkv=qkv, wq=wq, wk=wk, cos=cos, sin=sin, pos=pos, Hq=Hq, Hkv=Hkv,
            D=D):
        return C.qkv_norm_rope_fwd(qkv, wq, wk, cos, sin, pos, Hq, Hkv, D,
                                   EPS)

    def bwd(dq=dq, dk=dk, dv=dv, qkv=qkv, wq=wq, wk=wk, cos=cos, sin=sin,
            pos=pos):
        return C.qkv_norm_rope_bwd(dq, dk, dv, qkv, wq, wk, cos, sin, pos,
                                   EPS)

    cos32, sin32 = tables(32, MAX_POS, "cuda")
    bad = [
        lambda: fwd(qkv=qkv.float()),                       # dtype
        lambda: fwd(wq=wq.float()),
        lambda: fwd(cos=cos.double()),
        lambda: fwd(pos=pos.long()),
        lambda: fwd(qkv=qkv.cpu()),                         # device
        lambda: fwd(wk=wk.cpu()),
        lambda: fwd(sin=sin.cpu()),
        lambda: fwd(pos=pos.cpu()),
        lambda: fwd(qkv=qkv.transpose(0, 1)),               # contiguity
        lambda: fwd(qkv=qkv[0]),                            # shape
        lambda: fwd(qkv=qkv[..., :-D].contiguous()),        # W mismatch
        lambda: fwd(Hq=Hq + 1),
        lambda: fwd(wq=wq[:-1].contiguous()),
        lambda: fwd(cos=cos[:, :-1].contiguous()),          # table width
        lambda: fwd(pos=pos[:-1].contiguous()),             # positions [S]
        lambda: fwd(pos=None, cos=cos[:S - 1].contiguous(),
                    sin=sin[:S - 1].contiguous()),          # table too short
        lambda: fwd(qkv=torch.zeros(B, S, (Hq + 2 * Hkv) * 32, device="cuda",
                                    dtype=torch.bfloat16),
                    wq=wq[:32].contiguous(), wk=wk[:32].contiguous(),
                    cos=cos32, sin=sin32, D=32),            # D = 32
        lambda: bwd(dq=dq.float()),
        lambda: bwd(dk=dk.cpu()),
        lambda: bwd(dv=dv[:, :-1].contiguous()),
        lambda: bwd(dq=dq[:, :-1].contiguous(), dk=dk[:, :-1].contiguous(),
                    dv=dv[:, :-1].contiguous()),            # S != qkv's
        lambda: bwd(qkv=qkv[..., :-D].contiguous()),
        lambda: bwd(wk=wk.float()),
        lambda: bwd(pos=pos[:-1].contiguous()),
        lambda: bwd(dq=torch.zeros(B, S, Hq, 32, device="cuda",
                                   dtype=torch.bfloat16),
                    dk=torch.zeros(B, S, Hkv, 32, device="cuda",
                                   dtype=torch.bfloat16),
                    dv=torch.zeros(B, S, Hkv, 32, device="cuda",
                                   dtype=torch.bfloat16),
                    qkv=torch.zeros(B, S, (Hq + 2 * Hkv) * 32, device="cuda",
                                    dtype=torch.bfloat16),
                    wq=wq[:32].contiguous(), wk=wk[:32].contiguous(),
                    cos=cos32, sin=sin32),                  # D = 32
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"bad call #{i} was accepted")
    # a well-formed call afterwards still works
    assert_qk_close(_run(inp, cos, sin, pos, Hq, Hkv, D), ref, "after checks")


# --------------------------------------------------------------------------
# qwen3-debug through the kernel path
# --------------------------------------------------------------------------
def test_qwen3_debug_matches_cpu_fp32():
    from distributed_training_guide_amd.models import build_model

    torch.manual_seed(7)
    model = build_model("qwen3-debug", device=torch.device("cuda"),
                        dtype=torch.bfloat16)
    # QK-norm weights off 1, so the weight path carries information
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".q_norm." in n or ".k_norm." in n:
                p.copy_(1.0 + 0.3 * torch.randn_like(p))
    cpu = build_model("qwen3-debug", device=torch.device("cpu"),
                      dtype=torch.float32)
    cpu.load_state_dict({k: v.float().cpu()
                         for k, v in model.state_dict().items()})
    ids = torch.randint(0, 1024, (2, 96), device="cuda")
    out = model(input_ids=ids, labels=ids)
    out_cpu = cpu(input_ids=ids.cpu(), labels=ids.cpu())
    rel = abs(out.loss.item() - out_cpu.loss.item()) / out_cpu.loss.item()
    print(f"GPU bf16 loss {out.loss.item()} CPU fp32 {out_cpu.loss.item()} "
          f"rel {rel:.3e}")
    assert rel < 3e-2
    out.loss.backward()
    for n, p in model.named_parameters():
        assert p.grad is not None, n
        assert torch.isfinite(p.grad.float()).all(), n
        if ".q_norm." in n or ".k_norm." in n:
            assert p.grad.float().abs().max() > 0, n


def test_qwen3_debug_converges_on_fixed_batch():
    from distributed_training_guide_amd.models import build_model
    from distributed_training_guide_amd.ops import FusedAdamW

    torch.manual_seed(0)
    model = build_model("qwen3-debug", device=torch.device("cuda"),
                        dtype=torch.bfloat16)
    # the learning rate of test_loss_converges_on_fixed_batch
    opt = FusedAdamW(model.parameters(), lr=3e-4)
    ids = torch.randint(0, 1024, (4, 256), device="cuda")
    first = last = None
    for step in range(40):
        out = model(input_ids=ids, labels=ids)
        loss = out.loss.item()
        first = loss if first is None else first
        last = loss
        assert loss == loss, f"loss NaN at step {step}"
        out.loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    print(f"loss {first} -> {last}")
    assert last < first * 0.5, f"loss {first} -> {last}: not converging"


def test_qwen3_debug_fp8_forward_backward_finite():
    from distributed_training_guide_amd.models import build_model
    from distributed_training_guide_amd.ops import convert_linears_to_fp8

    torch.manual_seed(1)
    model = build_model("qwen3-debug", device=torch.device("cuda"),
                        dtype=torch.bfloat16)
    names = convert_linears_to_fp8(model)
    assert "layers.0.self_attn.qkv_proj" in names
    ids = torch.randint(0, 1024, (2, 64), device="cuda")
    loss = model(input_ids=ids, labels=ids).loss
    loss.backward()
    assert torch.isfinite(loss).item()
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad.float()).all(), n
