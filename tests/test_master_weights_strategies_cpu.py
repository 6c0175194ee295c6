"""--master-weights through the sharded strategies on CPU (world 2, gloo):
the chapters start, log the companions, step, and their sharded checkpoints
carry master_lo as int16; the ZeRO-3 engine takes the option from its config
and resumes from its checkpoint bit for bit."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from utils_dist import free_port, run_dist

REPO = Path(__file__).resolve().parent.parent


def _torchrun(chapter, tmp_path, extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
              "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(free_port()),
         str(REPO / chapter / "train_llm.py"), "-m", "llama-debug",
         "-d", "synthetic", "-s", "64", "-b", "2", "--num-samples", "32",
         "--num-workers", "0", "--log-freq", "1", "--device", "cpu",
         "--max-steps", "2", "--num-epochs", "1", "--save-dir",
         str(tmp_path), "-e", "mw", "--ckpt-freq", "2", "--master-weights",
         *extra],
        capture_output=True, text=True, timeout=420, cwd=REPO, env=env)


@pytest.mark.parametrize("chapter", ["02-distributed-data-parallel",
                                     "04-fully-sharded-data-parallel",
                                     "06-tensor-parallel"])
def test_chapter_trains_and_checkpoints_with_master_weights(tmp_path,
                                                            chapter):
    out = _torchrun(chapter, tmp_path, [])
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-2500:])
    m = re.search(r"Master weights: (\d+) bf16 parameter tensors", out.stderr)
    assert m and int(m.group(1)) > 0, out.stderr[-2500:]
    assert "'global_step': 2" in out.stderr
    shards = sorted((tmp_path / "mw").rglob("shard_rank*.pt"))
    if chapter.startswith("02"):
        # chapter 2 drops the optimizer state under ZeRO-1 by design
        return
    assert len(shards) == 2
    for f in shards:
        osd = torch.load(f, map_location="cpu", weights_only=True)["optimizer"]
        los = [st["master_lo"] for st in osd["state"].values()]
        assert len(los) == int(m.group(1))
        assert all(t.dtype == torch.int16 for t in los)
        assert any(t.ne(0).any() for t in los)


def _factory(dtype):
    from distributed_training_guide_amd.models import build_model

    torch.manual_seed(0)
    return build_model("llama-debug", dtype=dtype)


def _engine_worker(rank, world, tmpdir):
    from distributed_training_guide_amd import engine as engine_mod

    config = {"master_weights": True,
              "optimizer": {"type": "AdamW", "params": {"lr": 1e-3}}}

    def steps(eng, first, n):
        for s in range(first, first + n):
            g = torch.Generator().manual_seed(100 * rank + s)
            ids = torch.randint(0, 1024, (2, 32), generator=g)
            eng.backward(eng(input_ids=ids, labels=ids).loss)
            eng.step()

    eng, opt, _, _ = engine_mod.initialize(
        config, model_factory=_factory, device=torch.device("cpu"))
    assert opt.master_weights is True
    steps(eng, 0, 2)
    los = [st["master_lo"] for st in opt.state.values()]
    assert los and all(t.dtype == torch.int16 for t in los)
    assert any(t.ne(0).any() for t in los)
    eng.save_checkpoint(tmpdir, {"epoch": 0})
    eng2, opt2, _, _ = engine_mod.initialize(
        config, model_factory=_factory, device=torch.device("cpu"))
    assert eng2.load_checkpoint(tmpdir) is not None
    steps(eng, 2, 1)
    steps(eng2, 2, 1)
    for u1, u2 in zip(eng.module.units, eng2.module.units):
        assert torch.equal(u1.shard.detach(), u2.shard.detach())
        assert torch.equal(opt.state[u1.shard]["master_lo"],
                           opt2.state[u2.shard]["master_lo"])

    # fp32 parameters: the option is a no-op
    eng3, opt3, _, _ = engine_mod.initialize(
        dict(config, bf16={"enabled": False}), model_factory=_factory,
        device=torch.device("cpu"))
    steps(eng3, 0, 1)
    assert opt3.master_summary() == (0, 0, 0)
    assert all("master_lo" not in st for st in opt3.state.values())


def test_engine_master_weights_resume(tmp_path):
    run_dist(_engine_worker, world_size=2, args=(str(tmp_path),))
