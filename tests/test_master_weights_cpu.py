"""16-bit-extended master weights without a GPU: the split / join rule, the
eager path of FusedAdamW(master_weights=True) against an fp32 parameter, the
state dict, the ZeRO-1 wrapper, the --master-weights flag and the compiler's
resource report for every adamw_kernel instantiation."""
import copy
import logging
import re
import shutil
import sys
from pathlib import Path

import pytest
import torch

from distributed_training_guide_amd.ops import (FusedAdamW, join_master,
                                                split_master)
from distributed_training_guide_amd.ops import adamw as adamw_mod

from utils_master import bits as _bits
from utils_master import i16 as _i16
from utils_master import i32 as _i32
from utils_master import run_stall

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))


def _finite_inputs():
    g = torch.Generator().manual_seed(0)
    parts = [torch.randn(2 ** 20, generator=g),
             _bits([0x00000000, 0x80000000]),                    # +-0
             _bits([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                    0x00008000, 0x00007FFF, 0x00400000]),        # denormals
             _bits([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF])]
    low = torch.arange(2 ** 16, dtype=torch.int64)
    for high in (0x3C23, 0x7F7F, 0x0000, 0x8000, 0xBF80, 0xFF7F, 0x0080):
        parts.append(_bits((high << 16) + low))
    return torch.cat(parts)


def test_split_join_are_exact_inverses():
    x = _finite_inputs()
    hi, lo = split_master(x)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.int16
    assert hi.shape == x.shape and lo.shape == x.shape
    back = join_master(hi, lo)
    assert back.dtype == torch.float32
    assert torch.equal(_i32(back), _i32(x))
    # the bf16 half against round-to-nearest-even: equal except at exact
    # ties (low half 0x8000), where it is the value farther from zero
    tie = (_i32(x).to(torch.int64) & 0xFFFF) == 0x8000
    assert tie.sum() >= 7
    rne = x.bfloat16()
    assert torch.equal(_i16(hi)[~tie], _i16(rne)[~tie])
    trunc = (_i32(x).to(torch.int64) & 0xFFFFFFFF) >> 16
    away = (trunc[tie] + 1)                      # magnitude bits + 1
    got = _i16(hi)[tie].to(torch.int64) & 0xFFFF
    assert torch.equal(got, away)
    # ... which differs from ties-to-even exactly where truncation is even
    differs = _i16(hi)[tie] != _i16(rne)[tie]
    assert torch.equal(differs, trunc[tie] % 2 == 0)
    assert lo[tie].eq(-32768).all()
    # a shape other than 1-D, and a non-contiguous input
    m = x[:4096].view(64, 64).t()
    h2, l2 = split_master(m)
    assert h2.shape == (64, 64)
    assert torch.equal(_i32(join_master(h2, l2)), _i32(m))


def test_split_join_nan():
    pats = [0x7FFF8000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00000, 0xFFC00000,
            0x7F800001, 0xFF800001, 0x7F808000, 0xFFFF8000, 0x7FFF7FFF]
    x = _bits(pats)
    assert torch.isnan(x).all()
    hi, lo = split_master(x)
    assert torch.isnan(hi).all()          # never the wrapped +-0 or +-inf
    assert (_i16(hi).to(torch.int64) & 0xFFFF).eq(0x7FC0).all()
    assert lo.eq(0).all()
    assert torch.isnan(join_master(hi, lo)).all()
    # neighbours of a NaN in one tensor are untouched
    y = torch.tensor([1.5, float("nan"), -2.25, float("inf")])
    h, l = split_master(y)
    j = join_master(h, l)
    assert torch.isnan(j[1]) and j[0] == 1.5 and j[2] == -2.25
    assert torch.isinf(j[3]) and torch.isinf(h[3])
    # largest finite fp32: bf16 shows inf, the master stays finite
    h, l = split_master(_bits([0x7F7FFFFF]))
    assert torch.isinf(h).all()
    assert torch.equal(_i32(join_master(h, l)), _i32(_bits([0x7F7FFFFF])))


def test_split_join_type_errors():
    with pytest.raises(TypeError):
        split_master(torch.zeros(4, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        join_master(torch.zeros(4), torch.zeros(4, dtype=torch.int16))
    with pytest.raises(TypeError):
        join_master(torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4))


# ---------------- the stall scenario ----------------
def test_stall_scenario_master_tracks_fp32_parameter():
    """200 steps at lr 3e-5: the master equals an fp32 parameter bit for bit
    after every step (asserted inside run_stall) and the visible bf16 values
    move.  Without master weights 99.8 % of the elements with |w| >= 2^-6
    never change."""
    frozen, frozen_plain = run_stall("cpu", 200)
    print(f"frozen among |w| >= 2^-6: master {frozen:.4f}, "
          f"plain bf16 {frozen_plain:.4f}")
    assert frozen < 0.01
    assert frozen_plain > 0.9       # the problem this option removes


# ---------------- option off ----------------
def _two_params(seed=3):
    g = torch.Generator().manual_seed(seed)
    a = torch.nn.Parameter(torch.randn(33, 7, generator=g).bfloat16())
    b = torch.nn.Parameter(torch.randn(19, generator=g))
    return [a, b]


def _step_n(opt, params, n, first=0):
    for s in range(first, first + n):
        g = torch.Generator().manual_seed(50 + s)
        for p in params:
            p.grad = torch.randn(p.shape, generator=g).to(p.dtype)
        opt.step()


def test_option_off_is_unchanged():
    pa, pb, pc = _two_params(), _two_params(), _two_params()
    oa = FusedAdamW(pa, lr=1e-2)
    ob = FusedAdamW(pb, lr=1e-2, master_weights=False)
    oc = FusedAdamW(pc, lr=1e-2, master_weights=True)
    _step_n(oa, pa, 5)
    _step_n(ob, pb, 5)
    _step_n(oc, pc, 5)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
        assert set(ob.state[y]) == {"exp_avg", "exp_avg_sq"}
        assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"])
        assert torch.equal(ob.master_param(y), y.detach().float())
    assert oa.state_dict()["param_groups"] == ob.state_dict()["param_groups"]
    # with the option on only the bf16 parameter has a companion, and the
    # fp32 parameter steps exactly as before
    assert "master_lo" in oc.state[pc[0]]
    assert "master_lo" not in oc.state[pc[1]]
    assert torch.equal(pc[1], pa[1])
    assert torch.equal(oc.master_param(pc[1]), pc[1].detach())
    assert oc.master_summary() == (1, 33 * 7, 2 * 33 * 7)
    assert oa.master_summary() == (0, 0, 0)


# ---------------- state dict ----------------
def test_state_dict_round_trip_and_resume(tmp_path):
    straight = _two_params()
    o1 = FusedAdamW(straight, lr=1e-2, master_weights=True)
    _step_n(o1, straight, 6)

    first = _two_params()
    o2 = FusedAdamW(first, lr=1e-2, master_weights=True)
    _step_n(o2, first, 3)
    sd = o2.state_dict()
    assert sd["state"][0]["master_lo"].dtype == torch.int16
    assert "master_lo" not in sd["state"][1]
    torch.save({"opt": sd, "params": [p.detach() for p in first]},
               tmp_path / "ck.pt")
    blob = torch.load(tmp_path / "ck.pt", weights_only=True)
    assert blob["opt"]["state"][0]["master_lo"].dtype == torch.int16

    second = [torch.nn.Parameter(t.clone()) for t in blob["params"]]
    o3 = FusedAdamW(second, lr=1e-2, master_weights=True)
    o3.load_state_dict(blob["opt"])
    lo = o3.state[second[0]]["master_lo"]
    assert lo.dtype == torch.int16 and lo.shape == second[0].shape
    assert torch.equal(lo, o2.state[first[0]]["master_lo"])
    assert lo.data_ptr() != blob["opt"]["state"][0]["master_lo"].data_ptr()
    _step_n(o3, second, 3, first=3)
    for x, y in zip(straight, second):
        assert torch.equal(x, y)
        assert torch.equal(_i32(o1.master_param(x)), _i32(o3.master_param(y)))
        for k in o1.state[x]:
            assert torch.equal(o1.state[x][k], o3.state[y][k]), k


def test_load_state_without_master_lo_starts_from_zeros():
    old = _two_params()
    o_old = FusedAdamW(old, lr=1e-2)
    _step_n(o_old, old, 2)
    new = [torch.nn.Parameter(p.detach().clone()) for p in old]
    o_new = FusedAdamW(new, lr=1e-2, master_weights=True)
    saved = copy.deepcopy(o_old.state_dict())   # load does not copy fp32
    o_new.load_state_dict(copy.deepcopy(saved))
    assert "master_lo" not in o_new.state[new[0]]
    assert torch.equal(o_new.master_param(new[0]), new[0].detach().float())
    _step_n(o_new, new, 1, first=2)
    lo = o_new.state[new[0]]["master_lo"]
    assert lo.dtype == torch.int16
    # one step from a zero companion = one step of the widened value
    ref = [torch.nn.Parameter(old[0].detach().float())]
    o_ref = FusedAdamW(ref, lr=1e-2)
    o_ref.load_state_dict({"state": {0: saved["state"][0]},
                           "param_groups": [dict(saved["param_groups"][0],
                                                 params=[0])]})
    g = torch.Generator().manual_seed(52)
    ref[0].grad = torch.randn(ref[0].shape, generator=g).bfloat16().float()
    o_ref.step()
    assert torch.equal(_i32(o_new.master_param(new[0])), _i32(ref[0].detach()))


def test_load_state_with_master_lo_into_plain_optimizer(caplog):
    src = _two_params()
    o_src = FusedAdamW(src, lr=1e-2, master_weights=True)
    _step_n(o_src, src, 2)
    dst = [torch.nn.Parameter(p.detach().clone()) for p in src]
    o_dst = FusedAdamW(dst, lr=1e-2)
    with caplog.at_level(logging.WARNING, logger=adamw_mod.__name__):
        o_dst.load_state_dict(o_src.state_dict())
    lines = [r for r in caplog.records if "master_lo" in r.getMessage()]
    assert len(lines) == 1
    for p in dst:
        assert set(o_dst.state[p]) == {"exp_avg", "exp_avg_sq"}
    _step_n(o_dst, dst, 1, first=2)      # and it steps
    assert "master_lo" not in o_dst.state[dst[0]]


def test_reset_master():
    ps = _two_params()
    opt = FusedAdamW(ps, lr=1e-2, master_weights=True)
    _step_n(opt, ps, 2)
    assert opt.state[ps[0]]["master_lo"].ne(0).any()
    with torch.no_grad():
        ps[0].copy_(torch.ones_like(ps[0]))   # overwritten from outside
    opt.reset_master()
    assert opt.state[ps[0]]["master_lo"].eq(0).all()
    assert torch.equal(opt.master_param(ps[0]), torch.ones(33, 7))


# ---------------- ZeRO-1 wrapper ----------------
def test_zero1_forwards_master_weights(tmp_path):
    import torch.distributed as dist

    from distributed_training_guide_amd.parallel.zero1 import \
        ZeroRedundancyOptimizer

    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg",
                            rank=0, world_size=1)
    try:
        ps, ref = _two_params(), _two_params()
        z = ZeroRedundancyOptimizer(ps, optimizer_class=FusedAdamW, lr=1e-2,
                                    master_weights=True)
        assert z.local_opt.master_weights is True
        o = FusedAdamW(ref, lr=1e-2, master_weights=True)
        _step_n(z, ps, 3)
        _step_n(o, ref, 3)
        assert z.state[ps[0]]["master_lo"].dtype == torch.int16
        for x, y in zip(ps, ref):
            assert torch.equal(x, y)
        assert "master_lo" in z.state_dict()["state"][0]
    finally:
        dist.destroy_process_group()


# ---------------- trainer ----------------
def test_trainer_runs_with_master_weights(tmp_path, capfd):
    from distributed_training_guide_amd.parallel.single import \
        SingleDeviceStrategy
    from distributed_training_guide_amd.trainer import (get_parser,
                                                        run_training)

    assert get_parser().parse_args(["-m", "x"]).master_weights is False
    torch.manual_seed(0)
    args = get_parser().parse_args([
        "-m", "llama-debug", "-d", "synthetic", "-s", "64", "-b", "2",
        "--num-samples", "2", "--num-workers", "0", "--log-freq", "1",
        "--save-dir", str(tmp_path), "--num-epochs", "8", "--max-steps", "8",
        "--device", "cpu", "--lr", "1e-3", "--master-weights",
        "-e", "mw", "--ckpt-freq", "8"])
    state = run_training(args, SingleDeviceStrategy(args))
    assert state["global_step"] == 8
    err = capfd.readouterr().err
    m = re.search(r"Master weights: (\d+) bf16 parameter tensors \((\d+) "
                  r"elements\)", err)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0
    # one batch per epoch, the same two rows every step
    losses = [float(x) for x in re.findall(
        r"\{'global_step': \d+, 'lr': [^,]+, 'running_loss': ([^,]+),", err)]
    assert len(losses) == 8, err[-2000:]
    assert all(torch.isfinite(torch.tensor(losses)))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    # the unsharded checkpoint carries the companions as int16
    osd = torch.load(tmp_path / "mw" / "optimizer.pt", weights_only=True)
    los = [st["master_lo"] for st in osd["state"].values()]
    assert len(los) == int(m.group(1))
    assert all(t.dtype == torch.int16 for t in los)
    assert any(t.ne(0).any() for t in los)


# ---------------- compiler resources ----------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_adamw_kernels_use_no_scratch():
    import kernel_resources

    rows = kernel_resources.analyze(kernel_resources.HIP_DIR / "adamw.hip")
    by_name = {r["name"]: r for r in rows}
    expected = {f"adamw_kernel<{c}, {m}>" for c in ("false", "true")
                for m in ("false", "true")}
    assert set(by_name) == expected, sorted(by_name)
    for name, r in by_name.items():
        print(name, r["vgprs"], r["scratch"], r["occupancy"])
        assert r["scratch"] == 0, (name, r)
