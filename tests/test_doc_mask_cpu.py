"""Document-masked attention, CPU side: the doc_start / doc_end tables, the
fp32 reference, isolation of packed documents in the Llama model, the GPT-2
refusal, dataset rows, trainer flags and the TP model's plumbing."""
import math

import pytest
import torch

from utils_dist import run_dist

from distributed_training_guide_amd import ops
from distributed_training_guide_amd.ops import reference as R

EOS = 7


# ---------------- tables vs a plain loop ----------------
def _loop_tables(row, eos):
    S = len(row)
    start, cur = [], 0
    for i in range(S):
        if i > 0 and row[i - 1] == eos:
            cur = i
        start.append(cur)
    end = [S] * S
    for j in range(S):
        for i in range(j + 1, S):
            if start[i] != start[j]:
                end[j] = i
                break
    return start, end


LAYOUTS = {
    "eos_first": [[EOS, 1, 2, 3, 4, 5, 1, 2]],
    "eos_last": [[1, 2, 3, 4, 5, 6, 1, EOS]],
    "eos_run": [[1, 2, EOS, EOS, EOS, 3, 4, 5]],
    "no_eos": [[1, 2, 3, 4, 5, 6, 1, 2]],
    "batch2": [[1, EOS, 2, 3, EOS, 4, 5, 6], [EOS, EOS, 1, 2, 3, 4, 5, EOS]],
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_tables_match_loop(name):
    rows = LAYOUTS[name]
    ids = torch.tensor(rows)
    start = ops.doc_start_from_ids(ids, EOS)
    bounds = ops.doc_bounds(start)
    assert isinstance(bounds, ops.DocBounds)
    for t in (start, bounds.start, bounds.end):
        assert t.dtype == torch.int32 and t.is_contiguous()
        assert t.shape == ids.shape
    want = [_loop_tables(r, EOS) for r in rows]
    assert start.tolist() == [w[0] for w in want]
    assert bounds.start.tolist() == [w[0] for w in want]
    assert bounds.end.tolist() == [w[1] for w in want]
    ops.validate_doc_start(start)


def test_validator_rejects_broken_tables():
    ok = torch.tensor([[0, 0, 2, 2]], dtype=torch.int32)
    ops.validate_doc_start(ok)
    for bad in ([[0, 2, 2, 2]],     # doc_start[i] > i
                [[0, 1, 0, 0]],     # decreasing
                [[0, 0, 1, 1]]):    # doc_start[1] == 0, so 1 starts nothing
        with pytest.raises(ValueError):
            ops.validate_doc_start(torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.validate_doc_start(ok.long())


def test_flash_attention_rejects_bad_tables():
    q = torch.randn(1, 8, 2, 16)
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q, doc=torch.zeros(1, 8, dtype=torch.long))
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q, doc=torch.zeros(1, 7, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q, doc=[0] * 8)


# ---------------- reference: masked == per-document ----------------
def test_attention_ref_equals_per_document():
    torch.manual_seed(0)
    B, S, Hq, Hkv, D = 2, 40, 4, 2, 16
    q = torch.randn(B, S, Hq, D)
    k = torch.randn(B, S, Hkv, D)
    v = torch.randn(B, S, Hkv, D)
    scale = 1 / math.sqrt(D)
    lens = [[13, 1, 26], [40]]
    start = torch.zeros(B, S, dtype=torch.int32)
    for b, ls in enumerate(lens):
        at = 0
        for n in ls:
            start[b, at:at + n] = at
            at += n
    o = R.attention_ref(q, k, v, scale, doc_start=start)
    # the op's CPU path takes the same route, from either argument form
    assert torch.equal(ops.flash_attention(q, k, v, scale, doc=start), o)
    assert torch.equal(
        ops.flash_attention(q, k, v, scale, doc=ops.doc_bounds(start)), o)
    for b, ls in enumerate(lens):
        at = 0
        for n in ls:
            sl = slice(at, at + n)
            alone = R.attention_ref(q[b:b + 1, sl], k[b:b + 1, sl],
                                    v[b:b + 1, sl], scale)
            torch.testing.assert_close(o[b:b + 1, sl], alone)
            at += n
    # without doc_start the result is the plain causal one
    assert torch.equal(R.attention_ref(q, k, v, scale, doc_start=None),
                       R.attention_ref(q, k, v, scale))


# ---------------- model isolation ----------------
def _toy_llama():
    from distributed_training_guide_amd.models.llama import (
        LlamaConfig, LlamaForCausalLM)

    cfg = LlamaConfig(vocab_size=128, hidden_size=64, intermediate_size=128,
                      num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64,
                      initializer_range=0.3)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg, dtype=torch.float32)  # weights ~ N(0, 0.3)


def test_llama_packed_documents_are_isolated():
    model = _toy_llama()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 128, (1, 48), generator=g)
    start = torch.zeros(1, 48, dtype=torch.int32)
    start[0, 20:] = 20
    packed = model(input_ids=ids, doc_start=start).logits
    alone_a = model(input_ids=ids[:, :20]).logits
    alone_b = model(input_ids=ids[:, 20:],
                    position_ids=torch.arange(20, 48)).logits
    da = (packed[:, :20] - alone_a).abs().max().item()
    db = (packed[:, 20:] - alone_b).abs().max().item()
    print(f"doc A diff {da:.3e}, doc B diff {db:.3e}, "
          f"logit rms {packed.pow(2).mean().sqrt().item():.2f}")
    torch.testing.assert_close(packed[:, :20], alone_a, atol=1e-3, rtol=0)
    torch.testing.assert_close(packed[:, 20:], alone_b, atol=1e-3, rtol=0)
    # the mask is what isolates them: plain causal attention leaks
    leaky = model(input_ids=ids).logits
    assert (leaky[:, 20:] - alone_b).abs().max() > 0.1


def test_llama_no_gradient_across_documents():
    model = _toy_llama()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 128, (1, 48), generator=g)
    start = torch.zeros(1, 48, dtype=torch.int32)
    start[0, 20:] = 20
    seen = {}

    def keep(_module, _inputs, out):
        out.retain_grad()
        seen["x"] = out

    hook = model.embed_tokens.register_forward_hook(keep)
    logits = model(input_ids=ids, doc_start=start).logits
    hook.remove()
    logits[:, 20:].pow(2).sum().backward()
    gx = seen["x"].grad
    assert gx[:, 20:].abs().max() > 0
    assert torch.equal(gx[:, :20], torch.zeros_like(gx[:, :20]))


def test_doc_start_survives_activation_checkpointing():
    """The checkpoint wrapper forwards the layers' doc= keyword: the
    recompute sees the same mask, so the gradients are those of the plain
    run."""
    from distributed_training_guide_amd.parallel.fsdp import \
        apply_activation_checkpointing

    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 128, (1, 48), generator=g)
    start = torch.zeros(1, 48, dtype=torch.int32)
    start[0, 20:] = 20
    grads = []
    for ckpt in (False, True):
        model = _toy_llama()
        if ckpt:
            apply_activation_checkpointing(model)
        model(input_ids=ids, labels=ids, doc_start=start).loss.backward()
        grads.append([p.grad for p in model.parameters()])
    for a, b in zip(*grads):
        torch.testing.assert_close(a, b)


def test_gpt2_rejects_doc_start():
    from distributed_training_guide_amd.models.gpt2 import (GPT2Config,
                                                            GPT2ForCausalLM)

    model = GPT2ForCausalLM(GPT2Config(
        vocab_size=64, hidden_size=32, num_hidden_layers=1,
        num_attention_heads=2, max_position_embeddings=32))
    ids = torch.randint(0, 64, (1, 16))
    with pytest.raises(NotImplementedError, match="doc_start"):
        model(input_ids=ids, doc_start=torch.zeros(1, 16, dtype=torch.int32))
    model(input_ids=ids)  # still fine without


# ---------------- datasets ----------------
def test_packed_dataset_rows():
    from distributed_training_guide_amd.data.pipeline import PackedTokenDataset

    g = torch.Generator().manual_seed(0)
    stream = torch.randint(0, 12, (64,), generator=g, dtype=torch.int32)
    plain = PackedTokenDataset(stream, 16)
    off = PackedTokenDataset(stream, 16, eos_id=EOS, doc_mask=False)
    on = PackedTokenDataset(stream, 16, eos_id=EOS, doc_mask=True)
    assert len(plain) == len(on) == 4
    for i in range(4):
        a, b, c = plain[i], off[i], on[i]
        assert list(a) == list(b) == ["input_ids", "attention_mask", "labels"]
        assert list(c) == list(a) + ["doc_start"]
        for key in a:
            assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key])
        want = ops.doc_start_from_ids(c["input_ids"][None], EOS)[0]
        assert c["doc_start"].dtype == torch.int32
        assert torch.equal(c["doc_start"], want)
        ops.validate_doc_start(c["doc_start"][None])
    with pytest.raises(ValueError):
        PackedTokenDataset(stream, 16, doc_mask=True)


def test_synthetic_dataset_rows():
    from distributed_training_guide_amd.data import (SyntheticTextDataset,
                                                     default_collate)

    plain = SyntheticTextDataset(100, 64, num_samples=4, seed=3)
    same = SyntheticTextDataset(100, 64, num_samples=4, seed=3, doc_len=0)
    docs = SyntheticTextDataset(100, 64, num_samples=4, seed=3, doc_len=8,
                                doc_mask=True)
    n_eos = 0
    for i in range(4):
        a, b, c = plain[i], same[i], docs[i]
        assert list(a) == list(b) == ["input_ids", "attention_mask", "labels"]
        for key in a:
            assert torch.equal(a[key], b[key])
        assert list(c) == list(a) + ["doc_start"]
        # deterministic per (seed, index)
        assert torch.equal(docs[i]["input_ids"], c["input_ids"])
        assert torch.equal(c["labels"], c["input_ids"])
        is_eos = c["input_ids"] == 99
        n_eos += int(is_eos.sum())
        # only EOS positions differ from the plain row
        assert torch.equal(c["input_ids"][~is_eos], a["input_ids"][~is_eos])
        want = ops.doc_start_from_ids(c["input_ids"][None], 99)[0]
        assert torch.equal(c["doc_start"], want)
    # mean gap 8 over 256 tokens: about 32 separators
    assert 16 <= n_eos <= 64
    batch = default_collate([docs[0], docs[1]])
    assert batch["doc_start"].shape == (2, 64)
    assert batch["doc_start"].dtype == torch.int32


def test_parser_exposes_flags():
    from distributed_training_guide_amd.trainer import get_parser

    args = get_parser().parse_args(["-m", "llama-debug"])
    assert args.doc_mask is False and args.synthetic_doc_len == 0
    args = get_parser().parse_args(["-m", "llama-debug", "--doc-mask",
                                    "--synthetic-doc-len", "64"])
    assert args.doc_mask is True and args.synthetic_doc_len == 64


def test_trainer_runs_with_doc_mask(tmp_path):
    import importlib
    import sys
    from pathlib import Path

    repo = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(repo / "01-single-gpu"))
    try:
        sys.modules.pop("train_llm", None)
        mod = importlib.import_module("train_llm")
        state = mod.main([
            "-m", "llama-debug", "-d", "synthetic", "-s", "32", "-b", "2",
            "--num-samples", "8", "--num-workers", "0", "--max-steps", "2",
            "-e", "doc-mask", "--save-dir", str(tmp_path), "--device", "cpu",
            "--num-epochs", "1", "--doc-mask", "--synthetic-doc-len", "8",
        ])
    finally:
        sys.path.remove(str(repo / "01-single-gpu"))
        sys.modules.pop("train_llm", None)
    assert state["global_step"] == 2


# ---------------- tensor parallel ----------------
def _tp_doc_parity(rank, world):
    from distributed_training_guide_amd.models import build_model, get_config
    from distributed_training_guide_amd.parallel.mesh import DeviceMesh2D
    from distributed_training_guide_amd.parallel.tp import TPLlamaForCausalLM

    mesh = DeviceMesh2D(tp_size=world)
    tp_model = TPLlamaForCausalLM(get_config("llama-debug"), mesh)
    torch.manual_seed(0)
    ref = build_model("llama-debug")
    torch.manual_seed(42)
    tp_model.init_weights()
    torch.manual_seed(42)
    ref.init_weights()

    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 1024, (2, 32), generator=g)
    start = torch.zeros(2, 32, dtype=torch.int32)
    start[0, 11:] = 11
    start[1, 5:] = 5
    start[1, 20:] = 20
    out_tp = tp_model(input_ids=ids, labels=ids, doc_start=start)
    out_ref = ref(input_ids=ids, labels=ids, doc_start=start)
    assert torch.allclose(out_tp.logits, out_ref.logits, atol=2e-4), \
        (out_tp.logits - out_ref.logits).abs().max()
    assert torch.allclose(out_tp.loss, out_ref.loss, atol=1e-4)
    # and the mask reached the attention layers at all
    plain = tp_model(input_ids=ids).logits
    assert not torch.allclose(out_tp.logits, plain, atol=2e-4)


def test_tp_forward_with_doc_start():
    run_dist(_tp_doc_parity, world_size=2)
