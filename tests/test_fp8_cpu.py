"""FP8 linears without a GPU: the eager reference path of ops/fp8_linear.py
(the same quantisation, then dequantise and multiply in fp32), the in-place
conversion, the --fp8 flag and its start-up checks, and checkpoint
interchange with bf16 models."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_training_guide_amd.models import build_model, get_config
from distributed_training_guide_amd.ops import (Fp8Linear,
                                                convert_linears_to_fp8,
                                                fp8_linear, fp8_quantize)
from distributed_training_guide_amd.trainer import (check_fp8_supported,
                                                    get_parser)

MKN = [(16, 16, 16), (64, 256, 128), (208, 80, 48), (128, 4096, 256)]


@pytest.mark.parametrize("M,K,N", MKN)
def test_reference_path_against_f_linear(M, K, N):
    """Relative Frobenius error of y, dx and dw against F.linear in fp64 on
    the same bf16 inputs: <= 0.05 where M*K >= 16384, 0.06 at (16, 16, 16)
    (tensor-wise e4m3 costs about 3.7 % per GEMM)."""
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).bfloat16().requires_grad_()
    w = (0.02 * torch.randn(N, K, generator=g)).bfloat16().requires_grad_()
    dy = torch.randn(M, N, generator=g).bfloat16()
    y = fp8_linear(x, w)
    y.backward(dy)
    xd = x.detach().double().requires_grad_()
    wd = w.detach().double().requires_grad_()
    F.linear(xd, wd).backward(dy.double())
    ref = dict(y=F.linear(xd, wd).detach(), dx=xd.grad, dw=wd.grad)
    got = dict(y=y.detach(), dx=x.grad, dw=w.grad)
    bound = 0.05 if M * K >= 16384 else 0.06
    for name in ("y", "dx", "dw"):
        assert got[name].dtype == torch.bfloat16
        assert got[name].shape == ref[name].shape
        err = ((got[name].double() - ref[name]).norm()
               / ref[name].norm()).item()
        print(name, err)
        assert 0.0 < err <= bound, (name, err)


def test_quantize_reference_values():
    x = torch.zeros(16, 32, dtype=torch.bfloat16)
    x[0, :7] = torch.tensor([17.0, 19.0, 447.0, 2.0 ** -10, 3 * 2.0 ** -10,
                             0.001, -0.0])
    x[15, 31] = -448.0
    q, qt, scale, inv_scale = fp8_quantize(x, transposed=True)
    assert scale.item() == 1.0 and inv_scale.item() == 1.0
    assert q.dtype == torch.float8_e4m3fn and qt.shape == (32, 16)
    assert torch.equal(qt.view(torch.uint8), q.view(torch.uint8).t())
    assert q[0, :7].float().tolist() == [16.0, 20.0, 448.0, 0.0, 2.0 ** -8,
                                         2.0 ** -9, 0.0]
    assert int(q.view(torch.uint8)[0, 6]) == 0x80  # -0 keeps its sign
    # all zeros: finite scales, zeros out
    q0, _, s0, i0 = fp8_quantize(torch.zeros(16, 16, dtype=torch.bfloat16))
    assert not q0.view(torch.uint8).any()
    assert torch.isfinite(s0) and torch.isfinite(i0)
    # a supplied scale is used and leaves inv_scale undefined
    q2, _, s2, i2 = fp8_quantize(x, scale=torch.tensor([2.0]))
    assert i2 is None and q2[0, 0].float().item() == 32.0  # 34 ties to 32
    # non-finite input is not hidden
    x[3, 3] = float("nan")
    qn, _, sn, _ = fp8_quantize(x)
    assert torch.isnan(sn) and torch.isnan(qn.float()).all()


def test_shape_and_dtype_errors():
    w = torch.zeros(32, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="multiples of 16"):
        fp8_linear(torch.zeros(24, 32, dtype=torch.bfloat16), w)
    with pytest.raises(ValueError, match="does not match"):
        fp8_linear(torch.zeros(32, 48, dtype=torch.bfloat16), w)
    with pytest.raises(TypeError, match="bf16"):
        fp8_linear(torch.zeros(32, 32), w)
    with pytest.raises(ValueError, match="multiples of 16"):
        fp8_quantize(torch.zeros(16, 24, dtype=torch.bfloat16))


class _Mixed(nn.Module):
    def __init__(self):
        super().__init__()
        kw = dict(dtype=torch.bfloat16)
        self.qkv_proj = nn.Linear(32, 96, bias=False, **kw)
        self.o_proj = nn.Linear(32, 32, bias=False, **kw)
        self.gate_up_proj = nn.Linear(32, 128, bias=False, **kw)
        self.down_proj = nn.Linear(64, 32, bias=False, **kw)
        self.biased = nn.Linear(32, 32, bias=True, **kw)
        self.odd_in = nn.Linear(24, 32, bias=False, **kw)
        self.odd_out = nn.Linear(32, 40, bias=False, **kw)
        self.lm_head = nn.Linear(32, 64, bias=False, **kw)


def test_conversion_swaps_exactly_the_projections():
    m = _Mixed()
    keys = list(m.state_dict().keys())
    params = [id(p) for p in m.parameters()]
    names = convert_linears_to_fp8(m)
    assert names == ["qkv_proj", "o_proj", "gate_up_proj", "down_proj"]
    for name, mod in m.named_children():
        assert (type(mod) is Fp8Linear) == (name in names), name
        assert isinstance(mod, nn.Linear)
    assert list(m.state_dict().keys()) == keys
    assert [id(p) for p in m.parameters()] == params
    assert convert_linears_to_fp8(m) == []  # already converted
    assert convert_linears_to_fp8(_Mixed(), skip=("lm_head", "o_proj")) == [
        "qkv_proj", "gate_up_proj", "down_proj"]


def test_conversion_of_llama_and_checkpoint_interchange():
    torch.manual_seed(0)
    bf16 = build_model("llama-debug", device="cpu", dtype=torch.bfloat16)
    fp8 = build_model("llama-debug", device="cpu", dtype=torch.bfloat16)
    names = convert_linears_to_fp8(fp8)
    L = get_config("llama-debug").num_hidden_layers
    assert names == [f"layers.{i}.{p}" for i in range(L)
                     for p in ("self_attn.qkv_proj", "self_attn.o_proj",
                               "mlp.gate_up_proj", "mlp.down_proj")]
    assert type(fp8.lm_head) is nn.Linear
    assert list(fp8.state_dict().keys()) == list(bf16.state_dict().keys())
    # a bf16 checkpoint into the converted model, and back
    fp8.load_state_dict(bf16.state_dict(), strict=True)
    back = build_model("llama-debug", device="cpu", dtype=torch.bfloat16)
    back.load_state_dict(fp8.state_dict(), strict=True)
    for (k, a), (_, b) in zip(bf16.state_dict().items(),
                              back.state_dict().items()):
        assert torch.equal(a, b), k
    ids = torch.randint(0, 1024, (2, 64))
    ref = bf16(input_ids=ids, labels=ids).loss
    out = fp8(input_ids=ids, labels=ids)
    out.loss.backward()
    assert torch.isfinite(out.loss)
    assert out.loss.item() != ref.item()          # the fp8 path did run
    assert abs(out.loss.item() - ref.item()) < 0.05
    for name, p in fp8.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_fp8_flag_parses():
    assert get_parser().parse_args(["-m", "llama-debug"]).fp8 is False
    assert get_parser().parse_args(["-m", "llama-debug", "--fp8"]).fp8 is True


def test_fp8_start_up_errors():
    from distributed_training_guide_amd.parallel.ddp_strategy import \
        DDPStrategy
    from distributed_training_guide_amd.parallel.fsdp_strategy import \
        FSDPStrategy
    from distributed_training_guide_amd.parallel.single import \
        SingleDeviceStrategy
    from distributed_training_guide_amd.parallel.tp_strategy import (
        TPStrategy, TwoDStrategy)

    llama, gpt2 = get_config("llama-debug"), get_config("gpt2")
    check_fp8_supported(llama, SingleDeviceStrategy)
    check_fp8_supported(llama, DDPStrategy)
    for strategy in (FSDPStrategy, TPStrategy, TwoDStrategy):
        with pytest.raises(ValueError, match=f"--fp8 is not supported with "
                                             f"{strategy.__name__}"):
            check_fp8_supported(llama, strategy)
    with pytest.raises(ValueError, match="--fp8 is not supported for model "
                                         "type 'gpt2'"):
        check_fp8_supported(gpt2, SingleDeviceStrategy)


def _run_trainer(tmp_path, model, extra):
    from distributed_training_guide_amd.parallel.single import \
        SingleDeviceStrategy
    from distributed_training_guide_amd.trainer import run_training

    args = get_parser().parse_args([
        "-m", model, "-d", "synthetic", "-s", "64", "-b", "2",
        "--num-samples", "32", "--num-workers", "0", "--log-freq", "1",
        "--save-dir", str(tmp_path), "--num-epochs", "1", "--max-steps", "2",
        "--device", "cpu",
    ] + extra)
    return run_training(args, SingleDeviceStrategy(args))


def test_trainer_runs_with_fp8(tmp_path, capfd):
    state = _run_trainer(tmp_path, "llama-debug", ["--fp8"])
    assert state["global_step"] == 2
    assert "FP8 (e4m3) GEMMs in 16 linears" in capfd.readouterr().err


def test_trainer_rejects_fp8_for_gpt2(tmp_path):
    with pytest.raises(ValueError, match="model type 'gpt2'"):
        _run_trainer(tmp_path, "gpt2", ["--fp8"])


# ---------------- chapters under torchrun (world 2, gloo) ----------------
def _torchrun(chapter, tmp_path, extra):
    import os
    import subprocess
    import sys
    from pathlib import Path

    from utils_dist import free_port

    repo = Path(__file__).resolve().parent.parent
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
              "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(free_port()),
         str(repo / chapter / "train_llm.py"), "-m", "llama-debug",
         "-d", "synthetic", "-s", "64", "-b", "2", "--num-samples", "32",
         "--num-workers", "0", "--log-freq", "1", "--device", "cpu",
         "--max-steps", "2", "--num-epochs", "1", "--save-dir",
         str(tmp_path), *extra],
        capture_output=True, text=True, timeout=420, cwd=repo, env=env)


def test_ddp_chapter_trains_with_fp8(tmp_path):
    out = _torchrun("02-distributed-data-parallel", tmp_path, ["--fp8"])
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-2500:])
    assert "FP8 (e4m3) GEMMs in 16 linears" in out.stderr
    assert "'global_step': 2" in out.stderr


def test_fsdp_chapter_refuses_fp8(tmp_path):
    out = _torchrun("04-fully-sharded-data-parallel", tmp_path, ["--fp8"])
    assert out.returncode != 0
    assert "--fp8 is not supported with FSDPStrategy" in out.stderr
