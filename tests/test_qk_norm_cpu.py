"""QK-norm (ops/qk_norm.py) without a GPU: the eager op against fp64 per
element, the damage the bounds must reject, the Qwen3 model / registry
entries, tensor-parallel parity and a sharded trainer run."""
import math

import pytest
import torch

from utils_dist import run_dist
from utils_numerics import assert_bf16_close
from utils_qk_norm import (DAMAGES, EPS, MAX_POS, SHAPES, THETA,
                           assert_qk_close, cpu_case, qk_eval_f32)

QWEN3_SIZES = ("0.6b", "1.7b", "4b", "8b", "14b", "32b")


def _run_op(inp, Hq, Hkv, D, pos):
    from distributed_training_guide_amd.ops import qkv_norm_rope

    qkv = inp["qkv"].clone().requires_grad_(True)
    wq = inp["wq"].clone().requires_grad_(True)
    wk = inp["wk"].clone().requires_grad_(True)
    q, k, v = qkv_norm_rope(qkv, wq, wk, Hq, Hkv, D, EPS, theta=THETA,
                            positions=pos, max_pos=MAX_POS)
    torch.autograd.backward([q, k, v], [inp["dq"], inp["dk"], inp["dv"]])
    return dict(q=q.detach(), k=k.detach(), v=v.detach(), dqkv=qkv.grad,
                dwq=wq.grad, dwk=wk.grad)


@pytest.mark.parametrize("with_positions", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_eager_op_matches_fp64(shape, with_positions):
    B, S, Hq, Hkv, D = shape
    inp, cos, sin, pos, ref = cpu_case(shape, with_positions)
    got = _run_op(inp, Hq, Hkv, D, pos)
    for t in got.values():
        assert t.dtype == torch.bfloat16
    assert got["q"].shape == (B, S, Hq, D)
    assert got["k"].shape == got["v"].shape == (B, S, Hkv, D)
    assert_qk_close(got, ref, f"{shape} pos={with_positions}")
    # dv comes through the packed gradient unchanged
    assert torch.equal(got["dqkv"][..., (Hq + Hkv) * D:],
                       inp["dv"].reshape(B, S, Hkv * D))


@pytest.mark.parametrize("with_positions", [False, True])
def test_op_is_norm_then_rope(with_positions):
    """fp32 inputs: the op IS rope_ref(rmsnorm_ref(.)) on the q and k slices,
    norm first, and v passes through."""
    from distributed_training_guide_amd.ops import qkv_norm_rope
    from distributed_training_guide_amd.ops.reference import (rmsnorm_ref,
                                                              rope_ref)
    from distributed_training_guide_amd.ops.rope import get_rope_tables

    shape = SHAPES[1]
    B, S, Hq, Hkv, D = shape
    inp, _, _, pos, _ = cpu_case(shape, with_positions)
    qkv, wq, wk = inp["qkv"].float(), inp["wq"].float(), inp["wk"].float()
    q, k, v = qkv_norm_rope(qkv, wq, wk, Hq, Hkv, D, EPS, theta=THETA,
                            positions=pos, max_pos=MAX_POS)
    cos, sin = get_rope_tables(D, MAX_POS, THETA, qkv.device)
    xq, xk, xv = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    eq = rope_ref(rmsnorm_ref(xq.reshape(B, S, Hq, D), wq, EPS), cos, sin,
                  pos)
    ek = rope_ref(rmsnorm_ref(xk.reshape(B, S, Hkv, D), wk, EPS), cos, sin,
                  pos)
    assert torch.allclose(q, eq, rtol=0, atol=0)
    assert torch.allclose(k, ek, rtol=0, atol=0)
    assert torch.equal(v, xv.reshape(B, S, Hkv, D))
    # and not the other order
    wrong = rmsnorm_ref(rope_ref(xq.reshape(B, S, Hq, D), cos, sin, pos), wq,
                        EPS)
    assert not torch.allclose(q, wrong, atol=1e-3)


@pytest.mark.parametrize("shape", SHAPES)
def test_f32_evaluation_is_inside_the_bounds(shape):
    """What the kernel computes, evaluated in f32 on the CPU, passes: the
    bounds do not ask for more than f32 arithmetic gives."""
    B, S, Hq, Hkv, D = shape
    inp, cos, sin, pos, ref = cpu_case(shape, True)
    assert_qk_close(qk_eval_f32(inp, Hq, Hkv, D, cos, sin, pos), ref,
                    f"{shape} f32")


# which outputs each damage must push out of bound
_DAMAGED = {
    "no_eps": ("q", "dqkv"),            # the zero row: 0 * inf
    "rotate_first": ("q", "k"),
    "mean_without_weight": ("dqkv",),
    "dw_row_dropped": ("dwq", "dwk"),
    "truncate": ("q", "k", "dqkv"),
}


@pytest.mark.parametrize("damage", DAMAGES)
def test_damage_is_rejected(damage):
    shape = SHAPES[2]
    B, S, Hq, Hkv, D = shape
    inp, cos, sin, pos, ref = cpu_case(shape, True)
    bad = qk_eval_f32(inp, Hq, Hkv, D, cos, sin, pos, damage=damage)
    for key in _DAMAGED[damage]:
        with pytest.raises(AssertionError, match="out of bound"):
            assert_bf16_close(bad[key], ref[key], ref[key + "_mag"], key)


# --------------------------------------------------------------------------
# model and registry
# --------------------------------------------------------------------------
def _qk_norm_weights(model):
    return {n: p for n, p in model.named_parameters()
            if ".q_norm." in n or ".k_norm." in n}


def test_qwen3_debug_model():
    from distributed_training_guide_amd.models import build_model, get_config

    torch.manual_seed(0)
    cfg = get_config("qwen3-debug")
    assert cfg.qk_norm and cfg.head_dim == 128
    assert cfg.num_attention_heads * cfg.head_dim != cfg.hidden_size
    assert cfg.model_type == "llama"
    model = build_model(cfg)
    names = [n for n, _ in model.named_parameters()]
    assert "layers.0.self_attn.q_norm.weight" in names
    assert "layers.0.self_attn.k_norm.weight" in names
    assert sum(p.numel() for p in model.parameters()) == cfg.num_parameters()
    qk = _qk_norm_weights(model)
    assert len(qk) == 2 * cfg.num_hidden_layers
    for n, p in qk.items():
        assert p.shape == (128,) and torch.all(p == 1.0), n
    ids = torch.randint(0, cfg.vocab_size, (2, 16))
    out = model(input_ids=ids, labels=ids)
    assert math.isfinite(out.loss.item())
    assert abs(out.loss.item() - math.log(cfg.padded_vocab_size)) < 1.0
    out.loss.backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    for n, p in qk.items():
        assert p.grad.abs().max() > 0, n


def test_meta_init_leaves_qk_norm_weights_at_one():
    from distributed_training_guide_amd.models import get_config
    from distributed_training_guide_amd.models.llama import LlamaForCausalLM

    cfg = get_config("qwen3-debug")
    with torch.device("meta"):
        model = LlamaForCausalLM(cfg)
    model = model.to_empty(device="cpu")
    for p in model.parameters():
        with torch.no_grad():
            p.fill_(7.0)
    model.init_weights()
    for n, p in _qk_norm_weights(model).items():
        assert torch.all(p == 1.0), n
    ids = torch.randint(0, cfg.vocab_size, (1, 16))
    assert math.isfinite(model(input_ids=ids, labels=ids).loss.item())


def test_reset_param_by_name_fills_qk_norm_with_one():
    from distributed_training_guide_amd.models import build_model

    model = build_model("qwen3-debug")
    for name in ("layers.0.self_attn.q_norm.weight",
                 "layers.3.self_attn.k_norm.weight",
                 "layers.1.input_layernorm.weight", "norm.weight"):
        t = torch.full((128,), 7.0)
        model.reset_param_by_name(name, t)
        assert torch.all(t == 1.0), name
    t = torch.full((64, 64), 7.0)
    model.reset_param_by_name("layers.0.self_attn.qkv_proj.weight", t)
    assert t.std() < 0.1 and not torch.all(t == 1.0)


def test_existing_llama_models_are_unchanged():
    from distributed_training_guide_amd.models import build_model, get_config

    cfg = get_config("llama-debug")
    assert not cfg.qk_norm and cfg.head_dim == 64
    model = build_model(cfg)
    keys = set(model.state_dict())
    assert not any("q_norm" in k or "k_norm" in k for k in keys)
    per_layer = {"input_layernorm.weight", "post_attention_layernorm.weight",
                 "self_attn.qkv_proj.weight", "self_attn.o_proj.weight",
                 "mlp.gate_up_proj.weight", "mlp.down_proj.weight"}
    expect = {"embed_tokens.weight", "norm.weight", "lm_head.weight"} | {
        f"layers.{i}.{k}" for i in range(cfg.num_hidden_layers)
        for k in per_layer}
    assert keys == expect
    assert cfg.num_parameters() == sum(p.numel() for p in model.parameters())
    # the formula as it stood before head_dim could be set
    h, i, v = 256, 688, 1024
    assert cfg.num_parameters() == \
        (h * (4 + 2 * 2) * 64 + h * h + 3 * h * i + 2 * h) * 4 + 2 * v * h + h
    big = get_config("llama-3-8b")
    assert big.qk_norm is False and big.head_dim == 128
    assert big.num_parameters() == 8030261248
    # head_dim still follows an edited hidden_size
    cfg.hidden_size = 512
    assert cfg.head_dim == 128


@pytest.mark.parametrize("size", QWEN3_SIZES)
def test_qwen3_registry(size):
    from distributed_training_guide_amd.models import get_config

    base = get_config(f"qwen3-{size}")
    for alias in (f"Qwen/Qwen3-{size.upper()}", f"qwen/qwen3-{size}",
                  f"Qwen/Qwen3-{size.upper()}-Base"):
        cfg = get_config(alias)
        assert cfg == base, alias
    assert base.head_dim == 128 and base.qk_norm
    assert base.vocab_size == 151936 and base.rope_theta == 1e6
    assert base.rms_norm_eps == 1e-6
    assert base.max_position_embeddings == 40960
    assert base.num_key_value_heads == 8
    assert base.tie_word_embeddings == (size in ("0.6b", "1.7b", "4b"))


def test_unknown_model_message_lists_qwen3():
    from distributed_training_guide_amd.models import get_config

    with pytest.raises(ValueError, match="qwen3-8b.*qwen3-debug"):
        get_config("qwen3-9000b")


def test_gpu_head_dim_is_checked_before_anything_else():
    """The ValueError for an unsupported head dim is raised on the GPU path
    only; on the CPU any even head dim runs."""
    from distributed_training_guide_amd.ops import qkv_norm_rope

    qkv = torch.randn(1, 4, 4 * 32)
    w = torch.ones(32)
    q, k, v = qkv_norm_rope(qkv, w, w, 2, 1, 32, EPS)
    assert q.shape == (1, 4, 2, 32) and k.shape == v.shape == (1, 4, 1, 32)


# --------------------------------------------------------------------------
# tensor parallel
# --------------------------------------------------------------------------
def _batch(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (2, 32), generator=g)


def _tp_parity(rank, world):
    from distributed_training_guide_amd.models import build_model, get_config
    from distributed_training_guide_amd.parallel.mesh import DeviceMesh2D
    from distributed_training_guide_amd.parallel.tp import TPLlamaForCausalLM

    mesh = DeviceMesh2D(tp_size=world)
    cfg = get_config("qwen3-debug")
    tp_model = TPLlamaForCausalLM(cfg, mesh)
    torch.manual_seed(0)
    ref = build_model("qwen3-debug")
    torch.manual_seed(42)
    tp_model.init_weights()
    torch.manual_seed(42)
    ref.init_weights()
    # move the QK-norm weights off 1 (the same on every rank and in the
    # reference) so that a wrong weight or a wrong head shard would show
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for li, layer in enumerate(tp_model.layers):
            for name in ("q_norm", "k_norm"):
                w = 1.0 + 0.3 * torch.randn(128, generator=g)
                getattr(layer.self_attn, name).weight.copy_(w)
                getattr(ref.layers[li].self_attn, name).weight.copy_(w)

    ids = _batch()
    out_tp = tp_model(input_ids=ids, labels=ids)
    out_ref = ref(input_ids=ids, labels=ids)
    # the tolerances of test_tp_cpu.py
    assert torch.allclose(out_tp.logits, out_ref.logits, atol=2e-4), \
        (out_tp.logits - out_ref.logits).abs().max()
    assert torch.allclose(out_tp.loss, out_ref.loss, atol=1e-4)
    out_tp.loss.backward()
    out_ref.loss.backward()
    for li, layer in enumerate(tp_model.layers):
        for name in ("q_norm", "k_norm", "input_layernorm"):
            sub = layer if name == "input_layernorm" else layer.self_attn
            rsub = ref.layers[li] if name == "input_layernorm" \
                else ref.layers[li].self_attn
            gtp = getattr(sub, name).weight.grad
            gref = getattr(rsub, name).weight.grad
            assert gref.abs().max() > 0
            assert torch.allclose(gtp, gref, atol=1e-4), \
                f"layer {li} {name} grad {(gtp - gref).abs().max()}"
    # replicated in the grad-norm assembly, counted once
    (sharded, group), (repl, rgroup) = tp_model.grad_norm_parts()
    assert group is not None and rgroup is None
    repl_ids = {id(p) for p in repl}
    shard_ids = {id(p) for p in sharded}
    for layer in tp_model.layers:
        for name in ("q_norm", "k_norm"):
            w = getattr(layer.self_attn, name).weight
            assert id(w) in repl_ids and id(w) not in shard_ids
    # and in the checkpoint resharding rules
    name = "layers.0.self_attn.q_norm.weight"
    w = dict(tp_model.named_parameters())[name].detach()
    assert torch.equal(tp_model.shard_tensor(name, w), w)
    assert torch.equal(tp_model.reconstruct_full_tensor(name, [w, w]), w)


def test_tp_parity_with_single_process():
    run_dist(_tp_parity, world_size=2)


# --------------------------------------------------------------------------
# sharded strategies: meta-init and the trainer
# --------------------------------------------------------------------------
def _fsdp_meta_init_and_train(rank, world, tmpdir):
    import importlib
    import sys
    from pathlib import Path

    from distributed_training_guide_amd.models import build_model
    from distributed_training_guide_amd.parallel.fsdp import FSDP

    # before step 1: unit-by-unit meta materialisation leaves them at 1
    torch.manual_seed(0)
    with torch.device("meta"):
        model = build_model("qwen3-debug")
    fsdp = FSDP(model, device=torch.device("cpu"))
    full = fsdp.full_state_dict(rank0_only=False)
    qk = [n for n in full if ".q_norm." in n or ".k_norm." in n]
    assert len(qk) == 8, qk
    for n in qk:
        assert torch.all(full[n] == 1.0), n
    out = fsdp(input_ids=_batch(0), labels=_batch(0))
    assert abs(out.loss.item() - math.log(1024)) < 1.0
    del fsdp, model

    repo = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(repo / "04-fully-sharded-data-parallel"))
    mod = importlib.import_module("train_llm")
    state = mod.main([
        "-m", "qwen3-debug", "-d", "synthetic", "-s", "32", "-b", "1",
        "--num-samples", "16", "--num-workers", "0", "--max-steps", "2",
        "-e", "qk-fsdp", "--ckpt-freq", "2", "--save-dir", tmpdir,
        "--device", "cpu", "--num-epochs", "1",
    ])
    assert state["global_step"] == 2


def test_fsdp_trainer_two_steps(tmp_path):
    run_dist(_fsdp_meta_init_and_train, world_size=2, args=(str(tmp_path),))
    assert (tmp_path / "qk-fsdp" / "checkpoint" / "shard_rank0.pt").exists()


def _ddp_trainer(rank, world, tmpdir, extra):
    import importlib
    import sys
    from pathlib import Path

    repo = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(repo / "02-distributed-data-parallel"))
    mod = importlib.import_module("train_llm")
    state = mod.main([
        "-m", "qwen3-debug", "-d", "synthetic", "-s", "32", "-b", "1",
        "--num-samples", "16", "--num-workers", "0", "--max-steps", "2",
        "-e", "qk-ddp", "--ckpt-freq", "2", "--save-dir", tmpdir,
        "--device", "cpu", "--num-epochs", "1", *extra,
    ])
    assert state["global_step"] == 2


@pytest.mark.parametrize("extra", [(), ("--no-zero1",)],
                         ids=["zero1", "ddp"])
def test_ddp_trainer_two_steps(tmp_path, extra):
    """DDP with and without the ZeRO-1 optimizer, checkpoint included; the
    saved model carries the QK-norm weights under their HF names."""
    run_dist(_ddp_trainer, world_size=2, args=(str(tmp_path), extra))
    sd = torch.load(tmp_path / "qk-ddp" / "model.pt", weights_only=True)
    assert sd["layers.0.self_attn.q_norm.weight"].shape == (128,)
    assert sd["layers.3.self_attn.k_norm.weight"].shape == (128,)
